"""The word traces of tests/opwords.py hold what they promise, shown on the CPU oracle alone: without these conditions the GPU
tests of tests/test_gpu_opwords.py could pass vacuously (a block that never starts from its start, a reply code that never occurs,
a log ring that wraps).  Prints Lc, Lh and the trace sizes per workload (pytest -s)."""
import collections

import numpy as np
import pytest

import opwords as ow
from dint_amd import wire
from oracle import oracle as orc

W = wire.Workload
CASES = [(name, target) for name, spec in ow.SPECS.items() for target in spec.targets]
HOTS = [(n, t, True) for n, t in CASES] + [("smallbank", "saving", False), ("smallbank", "both", False)]
COLDS = [(n, t, lay) for n, t in CASES for lay in ow.layouts(ow.SPECS[n])]
IDS = lambda c: "-".join(str(x) for x in c)  # noqa: E731

# (request type, reply code) pairs every hot trace must draw from the oracle at least 20 times; lock_2pl: (action, type, reply)
PAIRS = {
    "lock_fasst": [(0, 4), (1, 5), (1, 6), (2, 7), (3, 8), (200, 200)],
    "lock_2pl": [(0, 0, 2), (0, 0, 3), (0, 1, 2), (0, 1, 3), (0, 9, 0), (1, 0, 5), (1, 1, 5), (1, 9, 5)],
    "store": [(0, 3), (0, 7), (1, 5), (1, 7), (2, 8), (77, 77)],
    "tatp": [(0, 4), (0, 6), (1, 7), (1, 8), (2, 9), (3, 3), (12, 15), (13, 16), (14, 17), (18, 20), (19, 21), (22, 25), (23, 26), (24, 27)],
    "smallbank": [(0, 7), (0, 8), (1, 9), (1, 10), (2, 11), (3, 12), (4, 13), (5, 14), (6, 15), (17, 18), (99, 99)],
}


def _codes(spec, req):
    if spec.wl == W.TPL:
        return (req["action"].astype(np.int64) << 4 | req["type"]).tolist()
    return req["type"].tolist()


def test_the_numpy_hashes_are_the_oracle_s():
    import struct

    for lid in (0, 1, 777, 2**32 - 1):
        assert int(ow.lid_slot([lid])[0]) == orc.fasthash64(struct.pack("<I", lid)) % ow.N_SLOTS
    for key in (7, 7 | (1 << 32), ow.SB_ABSENT):
        assert int(ow.lock_word([key], 1125)[0]) == orc.fasthash64(struct.pack("<Q", key)) % 4500


def test_de_bruijn_holds_every_window_once():
    for k, n in ((2, 3), (5, 5), (6, 4), (12, 3), (9, 3), (4, 6)):
        s = ow.de_bruijn(k, n)
        assert len(s) == k ** n + n - 1
        assert len({tuple(s[i:i + n]) for i in range(k ** n)}) == k ** n


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sizes(case):
    """Lc is the longest for which the batch stays within 65,536 requests, Lh the longest for which the hot trace stays below
    60,000; both are printed with the trace sizes (the table in the docstring of tests/opwords.py)"""
    name, target = case
    spec = ow.SPECS[name]
    c, h = ow.cold(name, target), ow.hot(name, target)
    rep, a = len(ow.tables_of(spec, target)), len(spec.alphabet)
    assert len(c.adjacent) == rep * len(spec.starts) * sum(a ** k * k for k in range(1, c.L + 1)) <= ow.COLD_MAX
    assert len(c.adjacent) + rep * len(spec.starts) * a ** (c.L + 1) * (c.L + 1) > ow.COLD_MAX
    assert len(h.req) < ow.HOT_MAX <= rep * len(ow.hot_starts(spec)) * a ** (h.L + 1) * (h.L + 1)  # (the next length's words alone)
    assert h.L <= c.L  # the cold replay classifies every hot block
    if name == "tatp":
        assert c.L >= 3
    print(f"\n{name:10s} {target:16s} Lc {c.L} cold words {len(c.blocks):6d} requests {len(c.adjacent):6d} preamble {len(c.pre):6d} | "
          f"Lh {h.L} hot requests {len(h.req):6d} front {h.n_front:5d} tail {h.n_tail:5d}")
    if name == "smallbank":
        g = ow.hot(name, target, False)
        print(f"{'':27s} row absent: Lh {g.L} hot requests {len(g.req):6d} front {g.n_front:5d} tail {g.n_tail:5d}")


@pytest.mark.parametrize("case", [("lock_2pl", "slot"), ("store", "row"), ("tatp", "call_forwarding"), ("smallbank", "both")], ids=IDS)
def test_the_builders_are_deterministic(case):
    name, target = case
    spec = ow.SPECS[name]
    h, c = ow.hot(name, target), ow.cold(name, target, "spread")
    h2, c2 = ow._build_hot(spec, target, True, h.L), ow.cold.__wrapped__(name, target, "spread")
    assert h2.req.tobytes() == h.req.tobytes() and h2.want.tobytes() == h.want.tobytes() and h2.blocks == h.blocks
    assert (h2.block_off == h.block_off).all() and (h2.word_off == h.word_off).all()
    for x in ("pre", "adjacent", "transposed"):
        assert getattr(c, x).tobytes() == getattr(c2, x).tobytes()
    assert (c.keys == c2.keys).all() and c.blocks == c2.blocks
    for d in (1, 7):
        assert ow.dilute(h, d)[0].tobytes() == ow.dilute(h, d)[0].tobytes()


@pytest.mark.parametrize("case", HOTS, ids=IDS)
def test_hot_trace_holds_every_block_once_from_its_start(case):
    """every (start, word) of length Lh exactly once; a fresh oracle that replays the trace is, at the first op of the word of a
    block in front of the tail, in the named start, and idle with the row the start wants at the block's first op: at the first and
    the last block and a sample of 250; the replies of that replay are the ones kept while the trace was built"""
    name, target, present = case
    spec = ow.SPECS[name]
    h = ow.hot(name, target, present)
    rep = len(ow.tables_of(spec, target))
    every = [(s, w) for s in ow.hot_starts(spec, present) for w in ow.words(spec, h.L)]
    assert sorted(h.blocks) == sorted(every) and len(set(h.blocks)) == len(every)
    codes = _codes(spec, h.req)
    for b, (start, word) in enumerate(h.blocks):  # the word's ops, where the offsets say
        at = int(h.word_off[b])
        assert tuple(codes[at:at + rep * h.L:rep]) == word and at + rep * h.L <= h.block_off[b + 1], b
    db = codes[int(h.block_off[-2]):int(h.block_off[-1]):rep]
    assert [spec.alphabet.index(x) for x in db] == ow.de_bruijn(len(spec.alphabet), h.L)
    sample = sorted({0, h.n_front - 1} | set(np.linspace(0, h.n_front - 1, 250).astype(int).tolist()))
    o = ow.oracle(spec)
    at, got = 0, []
    for b in sample:
        start = h.blocks[b][0]
        for off, want in ((int(h.block_off[b]), ow.idle_state(spec, start)), (int(h.word_off[b]), ow.start_state(spec, start))):
            got.append(o.replay(h.req[at:off]))
            at = off
            for t in ow.tables_of(spec, target):
                assert ow.in_state(spec, ow.slot_state(spec, o, t, h.key), want), (b, h.blocks[b], t)
    got.append(o.replay(h.req[at:]))
    assert np.concatenate(got).tobytes() == h.want.tobytes()
    assert getattr(o, "errors", 0) == h.errors
    if spec.wl in (W.TATP, W.SMALLBANK):  # the ring is larger than the trace's record count: DELETE_LOG's kept bytes are this trace's
        n_log = int(np.isin(h.req["type"], (14, 24) if spec.wl == W.TATP else (6,)).sum())
        assert o.tail == n_log < ow.LOG_CAP
    if h.n_tail:  # the tail is what no op leads back from, by the cold replay of the same word from its true start
        c = ow.cold(name, target)
        final = dict(zip(c.blocks, c.final_states()))
        for k, b in enumerate(h.blocks):
            assert (ow.fix_ops(spec, final[b], ow.idle_state(spec, b[0])) is None) == (k >= h.n_front), b


@pytest.mark.parametrize("case", HOTS, ids=IDS)
def test_hot_trace_draws_every_reply_code(case):
    name, target, present = case
    h = ow.hot(name, target, present)
    seen = collections.Counter(ow.reply_pairs(h.spec, h.req, h.want))
    short = {p: seen[p] for p in PAIRS[name] if seen[p] < 20}
    assert not short, short


@pytest.mark.parametrize("case", COLDS, ids=IDS)
def test_cold_traces_hold_every_word_once(case):
    """every (start, word) up to Lc exactly once, on a key of its own, in both arrangements; "spread": after the first submit
    every slot is in its start; the other layouts: the two keys of a pair share what the layout says"""
    name, target, layout = case
    spec = ow.SPECS[name]
    c = ow.cold(name, target, layout)
    rep = len(ow.tables_of(spec, target))
    every = [(s, w) for s in spec.starts for k in range(1, c.L + 1) for w in ow.words(spec, k)]
    assert sorted(c.blocks) == sorted(every) and len(set(c.blocks)) == len(every) == len(np.unique(c.keys))
    field = "lid" if ow.is_lock(spec) else "key"
    for arr in ("adjacent", "transposed"):
        req, blk = getattr(c, arr), c.block_of[arr]
        assert (req[field] == c.keys[blk].astype(req.dtype[field])).all()
        o = np.argsort(blk, kind="stable")  # the ops of a word in trace order
        codes, sb = np.array(_codes(spec, req))[o], blk[o]
        cut = np.searchsorted(sb, np.arange(len(c.blocks) + 1))
        for i in (0, 1, len(c.blocks) // 2, len(c.blocks) - 1) + tuple(range(7, len(c.blocks), 97)):
            assert tuple(codes[cut[i]:cut[i + 1]:rep]) == c.blocks[i][1], (arr, i)
        assert (np.diff(cut) == [rep * len(w) for _, w in c.blocks]).all()
    ops = [sorted(zip(_codes(spec, getattr(c, arr)), getattr(c, arr)[field].tolist())) for arr in ("adjacent", "transposed")]
    assert ops[0] == ops[1]  # the same ops on the same keys, in another order
    if layout == "spread":
        o = ow.oracle(spec, big=True)
        o.replay(c.pre)
        for t in ow.tables_of(spec, target):
            st = c.states(o, t)
            bad = [(b, s) for b, s in zip(c.blocks, st) if not ow.in_state(spec, s, ow.start_state(spec, b[0]))]
            assert not bad, bad[:3]
        if name == "smallbank":
            absent = np.array([s.endswith("-absent") for s, _ in c.blocks])
            assert (c.keys[absent] >= ow.POP_BIG).all() and (c.keys[~absent] < ow.POP_BIG).all()
        return
    if ow.is_lock(spec):
        s = ow.lid_slot(c.keys).reshape(-1, 2)
        if layout == "alias":
            assert (s[:, 0] == s[:, 1]).all()
        else:
            assert (s[:, 1] == s[:, 0] + 1).all() and (s[:, 0] // 16 == s[:, 1] // 16).all()
        assert len(np.unique(s[:, 0])) == len(s)
        return
    lw = ow.lock_word(c.keys, ow.oracle(spec, big=True).hash_size(ow.tables_of(spec, target)[0]))
    _, inv, cnt = np.unique(lw, return_inverse=True, return_counts=True)
    assert (cnt[inv] >= 2).sum() >= len(lw) - 1  # every word has another on its lock word (but one, where such rows run out)


@pytest.mark.parametrize("case", HOTS[:7], ids=IDS)
def test_dilution_leaves_the_hot_replies_alone(case):
    """the fillers touch other slots and rows and change nothing: the oracle's replies to the hot requests of a diluted trace are
    those of the plain one, so every block still starts from its start"""
    name, target, present = case
    h = ow.hot(name, target, present)
    for d in (1, 7):
        req, src = ow.dilute(h, d)
        assert len(req) == len(h.req) + d * (len(h.req) - 1) and (src[::d + 1] == np.arange(len(h.req))).all()
        o = ow.oracle(h.spec)
        rep = o.replay(req)
        assert rep[src >= 0].tobytes() == h.want.tobytes(), d
        fill = ow.reply_pairs(h.spec, req[src < 0], rep[src < 0])
        assert set(fill) <= {(0, 4), (0, 0, 2), (1, 0, 5), (0, 3), (17, 18)}, set(fill)  # granted reads / shared locks only


@pytest.mark.parametrize("name", ["lock_fasst", "lock_2pl", "tatp", "smallbank"])
def test_dual_traces_hold_both_traces_on_keys_that_share(name):
    spec = ow.SPECS[name]
    target = spec.targets[0]
    h = ow.hot(name, target)
    ka, kb = ow.dual_keys(name)
    if ow.is_lock(spec):
        sa, sb = ow.lid_slot([ka, kb])
        assert sb == sa + 1 and sa // 16 == sb // 16
    else:
        lw = ow.lock_word([ka, kb], ow.oracle(spec).hash_size(0))
        assert lw[0] == lw[1] and ka != kb and max(ka, kb) < ow.POP
    for ratio in (1, 20):
        req, src = ow.dual(name, target, ratio)
        field = "lid" if ow.is_lock(spec) else "key"
        a, b = req[field] == ka, req[field] == kb
        assert a.sum() == b.sum() == len(h.req) and len(req) == 2 * len(h.req)
        assert (src[a] == np.arange(len(h.req))).all() and sorted(src[b].tolist()) == list(range(len(h.req)))
        assert _codes(spec, req[a]) == _codes(spec, h.req)
        first = np.nonzero(b)[0][:40]
        assert (np.diff(first) == ratio + 1).all()
