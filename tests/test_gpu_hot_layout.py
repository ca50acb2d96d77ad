"""GPU parity of the kv and lock passes on hot keys whose requests bunch, thin out or sit at the edges of the pieces the passes cut
them into (kv_hot_item / kv_list_items, kv_sb_item, lk_big_bins): an empty piece, a piece of exactly 512 or 513 requests, a lone
refusing piece, a writer and its reader on either side of a range edge, a last writer at index 2^20 - 1, 8 against 9 foreign
requests, lock groups at 63 | 64 and 4095 | 4096, 65,536 COMMITs on one slot, counts on every threshold.  The traces, the oracle's
answers and the counter expectations come from tests/hotlayout.py (rules restated from the kernels, never from what the engine
reported); tests/test_hotlayout_host.py checks on the host that every trace holds what its layout promises.

Every case: a fresh populated engine under one knob set, the layout pass, then an ordinary pass on the same engine (the pieces'
words are tagged per pass: a stale one must not survive); every reply byte, rows in order, lock bytes / counters / lock words,
ring and tail, bad_requests and missing_keys equal the oracle's.  An "alone" case -- the hot sub holds the hot key's records and
nothing else -- also asserts the late counters, the only evidence that the intended branch ran: a layout the rules keep in closed
form leaves late_requests and late_items unchanged, one they refuse raises exactly the entries hotlayout.kv_counters names."""
import numpy as np
import pytest

import hotlayout as hl
from dint_amd import wire

pytestmark = pytest.mark.gpu
W = wire.Workload


def _differ(c, k, req, got, want):
    item = req.dtype.itemsize
    diff = (np.frombuffer(got.tobytes(), "u1") != np.frombuffer(want.tobytes(), "u1")).reshape(-1, item).any(axis=1)
    at = np.nonzero(diff)[0]
    hot = hl.hot_sel(c, k)
    pytest.fail(f"{c.name}: pass {k} of {len(req)}: {len(at)} replies differ from the oracle's ({int(hot[at].sum())} of them the hot key's), "
                f"first at requests {at[:8].tolist()}, types {req['type'][at[:8]].tolist()}")


@pytest.mark.parametrize("name,knobs", hl.runs(), ids=[f"{n}/{k}" for n, k in hl.runs()])
def test_hot_layout_vs_oracle(name, knobs, monkeypatch):
    from dint_amd.engine import Engine

    env, flags = hl.KNOBS[knobs]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = hl.case(name)
    eng = Engine(c.wl, flags=flags, **c.engine)
    if c.populate:
        eng.populate(c.populate)
    assert eng.pass_max >= c.n  # one pass
    counters = []
    for k, (req, want) in enumerate(zip(c.passes, c.want)):
        got = eng.submit(req)
        if got.tobytes() != want.tobytes():
            _differ(c, k, req, got, want)
        st = eng.stats()
        counters.append((st["late_requests"], list(st["late_items"][:3])))
    st = eng.stats()
    assert st["batches"] == 2 and st["pool_exhausted"] == 0
    if c.wl in hl.KV:
        for t, rows in enumerate(c.rows):
            assert hl.same_rows(eng.dump_rows(t), rows), ("rows differ", t)
        if c.wl == W.TATP:
            for t in range(5):
                assert (eng.read_locks(t)[0] == c.locks[t]).all(), ("lock bytes differ", t)
        elif c.wl == W.SMALLBANK:
            for t in range(2):
                ex, sh = eng.read_locks(t)
                assert (ex == c.locks[t][0]).all() and (sh == c.locks[t][1]).all(), ("lock counters differ", t)
        if c.wl != W.STORE:
            ring, tail = eng.read_log(c.log_cap)
            assert tail == c.tail and (np.frombuffer(ring.tobytes(), "u1").reshape(-1, 64) == c.ring).all()
        bad, missing = (c.errors, 0) if c.wl == W.STORE else (0, c.errors)
        assert (st["bad_requests"], st["missing_keys"]) == (bad, missing), (st["bad_requests"], st["missing_keys"], c.errors)
        assert c.wl != W.STORE or c.variant == "traffic" or st["bad_requests"] == c.bad == c.n - c.c - (6 if c.variant == "neighbour" else 0)
        if c.variant == "alone":
            want = hl.kv_counters(c, knobs)
            assert want is not None
            if c.foreign is None or hl.piece_counts(c, knobs)[1] == 0:
                assert counters[0] == want, (counters[0], want, hl.piece_counts(c, knobs)[:3])
            else:
                # two keys in the sub: which one the pieces are cut around falls to one sampled record (hotlayout.kv_counters) --
                # the hot row's almost surely, the foreign key's with probability its share of the sub (2 in 10,000 here)
                alt = hl.kv_counters(c, knobs, around="foreign")
                assert counters[0] in (want, alt), (counters[0], want, alt, "neither cut explains these counters")
    else:
        for got, (at, vals) in zip(eng.read_locks(), c.locks):
            assert np.count_nonzero(got) == len(at) and (got[at] == vals).all(), "lock words differ"
        assert st["bad_requests"] == c.errors
