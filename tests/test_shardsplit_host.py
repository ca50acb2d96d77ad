"""The shard projection of tests/shardsplit.py and the shard-aware placements of tests/opwords.py hold what they promise, shown on
the CPU oracle alone: without these conditions the GPU tests of tests/test_gpu_shard_words.py could pass vacuously (a projection
that drops a word, a shard that is sent nothing, an `edge` pair that is no edge).  Prints every GPU trace's size and its counts of
home and foreign requests per shard (pytest -s)."""
import numpy as np
import pytest

import kvkeys
import opwords as ow
import shardsplit as ss
from dint_amd import wire

W = wire.Workload
SIZES = [1, 5, 1125, 2812, 4218, 13_500, 9000, 1 << 20]  # the lock tables and the kv tables of the GPU cases (9000: tatp's, 24,000 rows)
HS = (2, 3, 8)


def _by_definition(a, size, i, H, quadrants):
    """the mapping restated request-wise: word q * size + g of the one server is word q * n_local + g // H of shard g % H"""
    nl = -(-size // H)
    out = np.zeros(quadrants * nl, a.dtype)
    for q in range(quadrants):
        for g in range(i, size, H):
            out[q * nl + g // H] = a[q * size + g]
    return out


def _check_partition(size, H, quadrants):
    rng = np.random.default_rng(size + H)
    a = rng.integers(1, 1 << 31, quadrants * size).astype("<u4")  # (no zero: a dropped word shows)
    seen = np.zeros(quadrants * size, np.int64)
    for i in range(H):
        src = ss.projection_index(size, i, H, quadrants)
        nl = ss.n_local(size, H)
        assert len(src) == quadrants * nl
        p = ss.project_kv_locks(a, size, i, H) if quadrants == 4 else ss.project_slots(a, a, size, i, H)[0]
        assert (p == np.where(src >= 0, a[np.maximum(src, 0)], 0)).all(), (size, H, i)
        if size <= 5000:
            assert (p == _by_definition(a, size, i, H, quadrants)).all(), (size, H, i)
        np.add.at(seen, src[src >= 0], 1)
        hole = (nl - 1) * H + i >= size  # the top local bucket of this shard corresponds to no global one
        assert ((src < 0).sum() == (quadrants if hole else 0)) and (not hole or (src.reshape(quadrants, nl)[:, -1] < 0).all())
        local, q = np.arange(quadrants * nl) % nl, np.arange(quadrants * nl) // nl
        ok = src >= 0
        assert (src[ok] == q[ok] * size + local[ok] * H + i).all()  # the claimed index
    assert (seen == 1).all(), (size, H)  # every word of the one server in exactly one shard


@pytest.mark.parametrize("H", HS + (255,))
def test_projections_partition_the_state(H):
    for size in SIZES:
        _check_partition(size, H, 1)
        if 5 < size < (1 << 20):
            _check_partition(size, H, 4)


def test_a_quadrant_mapped_with_n_local_less_one_is_caught(monkeypatch):
    """the mutation of the issue: project a quadrant's words with stride n_local - 1.  The partition check must notice"""
    true = ss.n_local
    _check_partition(1125, 2, 4)
    monkeypatch.setattr(ss, "_project", lambda a, size, i, H, quadrants: _mutated(a, size, i, H, quadrants, true))
    for H in (2, 8):
        with pytest.raises(AssertionError):
            _check_partition(1125, H, 4)


def _mutated(a, size, i, H, quadrants, n_local):
    nl = n_local(size, H)
    g = np.arange(i, size, H)
    out = np.zeros(quadrants * nl, np.asarray(a).dtype)
    for q in range(quadrants):
        at = q * (nl - 1)
        out[at:at + len(g)] = a[q * size + g][:len(out) - at]
    return out


@pytest.mark.parametrize("name", ["store", "tatp", "smallbank"])
@pytest.mark.parametrize("H", HS)
def test_projected_rows_partition_the_dump(name, H):
    spec = ow.SPECS[name]
    o = ow.oracle(spec)
    for t, hs in enumerate(ss.table_sizes(spec)):
        dump = o.dump() if spec.wl == W.STORE else o.dump(t)
        parts = [ss.project_rows(dump, hs, i, H) for i in range(H)]
        assert sum(len(p[0]) for p in parts) == len(dump[0]) > 0
        for i, (k, v, x) in enumerate(parts):
            g = kvkeys.np_bucket(k, hs).astype(np.int64)
            assert (g % H == i).all() and (np.diff(g // H) >= 0).all()  # the shard's own, in local bucket order
            at = np.nonzero(np.isin(dump[0], k))[0]
            assert (dump[0][at] == k).all() and (dump[1][at] == v).all() and (dump[2][at] == x).all()  # a subsequence: chain order kept
        assert len(np.unique(np.concatenate([p[0] for p in parts]))) == len(np.unique(dump[0]))


# ---- the placements --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["store", "tatp", "smallbank"])
@pytest.mark.parametrize("H", HS)
def test_edge_pairs_lie_on_the_edges(name, H):
    """bucket, quadrant, home, local index and group key of every `edge` pair, recomputed from the hash"""
    spec = ow.SPECS[name]
    c = ow.cold_edge(name, H)
    hs = ss.table_sizes(spec)
    nl = [ss.n_local(x, H) for x in hs]
    gk_base = np.concatenate([[0], np.cumsum(nl)])
    sig = [kvkeys.key_sig([k], hs[t]) for k, t in zip(c.keys, c.tables)]
    b, q = np.array([int(s[0][0]) for s in sig]), np.array([int(s[1][0]) for s in sig])
    t = c.tables
    local, gk, lw = b // H, gk_base[t] + b // H, q * np.array(nl)[t] + b // H
    kinds = {}
    for kind, i, x, y in c.pairs:
        kinds[kind] = kinds.get(kind, 0) + 1
        assert b[x] % H == b[y] % H == i  # one home
        assert local[x] == nl[t[x]] - 1 and b[x] + H >= hs[t[x]] and local[y] == 0 and b[y] == i  # the shard's greatest bucket | its least
        if kind == "cross":
            assert t[y] == t[x] + 1 and gk[y] == gk[x] + 1 and q[x] == q[y]  # adjacent group keys
        elif kind == "wrap":
            assert t[y] == t[x] == len(hs) - 1
        else:
            assert t[y] == t[x] and q[y] == (q[x] + 1) % 4 and (q[x] == 3 or lw[y] == lw[x] + 1)  # neighbouring lock words
    assert set(kinds) == ({"wrap", "quadrant"} if len(hs) == 1 else {"cross", "wrap", "quadrant"}), kinds
    tops = np.array([x for _, _, x, _ in c.pairs])
    _, n_on_word = np.unique((b[tops] % H * 8 + t[tops]) * (1 << 32) + lw[tops], return_counts=True)  # (per shard and table)
    assert (n_on_word == ow.EDGE_PER).all()  # two keys or more on every lock word of a top bucket
    assert {(tt, i) for tt, i in ow.edge_places(hs, H)} == {(int(t[x]), i) for _, i, x, _ in c.pairs}
    # what a table with n_local FLOORED would not hold: the top bucket's local index is hash_size // H wherever H leaves a remainder
    for tt, x in enumerate(hs):
        if x % H:
            assert (local[t == tt] == x // H).any(), (tt, x, H)
    every = {(s, w) for s in spec.starts for w in ow.words(spec, 1) if spec.wl != W.SMALLBANK or s.endswith("-absent")}
    assert every <= set(c.blocks) and len(set(c.blocks)) == len(c.blocks) == len(c.keys)
    o = ow.oracle(spec)
    o.replay(c.pre)  # after the preambles every word's row is what its start wants (the keys of a pair share lock words on purpose,
    for tt in sorted(set(t.tolist())):  # as those of "lockpair" do: a lock held for one word is held for its neighbours)
        sel = np.nonzero(t == tt)[0]
        for j in sel[:: max(1, len(sel) // 40)]:
            if spec.wl != W.SMALLBANK:
                assert ow.slot_state(spec, o, tt, int(c.keys[j]))[0] == ow.start_state(spec, c.blocks[j][0])[0], (j, c.blocks[j])
    held = sum(int((o.locks(tt) != 0).sum()) if spec.wl == W.TATP else int((o.num_ex(tt) + o.num_sh(tt) != 0).sum()) for tt in range(len(hs))) if spec.wl != W.STORE else 1
    assert held > 0
    print(f"\nedge {name:9s} H {H}: {len(c.blocks):4d} words, {len(c.pre):4d} + {len(c.adjacent):5d} requests, pairs {kinds}")


@pytest.mark.parametrize("name", ["lock_fasst", "lock_2pl"])
@pytest.mark.parametrize("H", HS)
def test_localline_pairs_share_a_local_line(name, H):
    c, c0 = ow.cold_localline(name, H), ow.cold(name, "slot")
    assert c.blocks == c0.blocks  # every word of the cold trace
    g = ow.lid_slot(c.keys)
    kinds = {"ends": 0, "line": 0}
    for kind, i, x, y in c.pairs:
        kinds[kind] += 1
        assert g[x] % H == g[y] % H == i
        if kind == "line":
            assert g[y] == g[x] + H and (g[x] // H) // 16 == (g[y] // H) // 16 and g[y] // H == g[x] // H + 1
        else:
            assert g[y] == i and g[x] + H >= ow.N_SLOTS and g[x] // H in (ss.n_local(ow.N_SLOTS, H) - 1, ss.n_local(ow.N_SLOTS, H) - 2)
    assert kinds["ends"] == H and kinds["line"] == len(c.blocks) // 2 - H
    assert len(np.unique(g)) == len(g)
    a, b = ow.lid_slot(list(ow.localline_dual_lids(3)))
    assert b == a + 3 and (a // 3) // 16 == (b // 3) // 16


# ---- every case of the GPU tests -----------------------------------------------------------------------------------------------------
CASES = ss.all_trace_cases()


@pytest.mark.parametrize("cid,make", CASES, ids=["-".join(str(x) for x in c) for c, _ in CASES])
def test_case_inputs_and_sub_stream_replay(cid, make):
    """no case is silently empty, and the commutation claim holds for it: fresh oracles that replay each shard's sub-stream alone
    give the replies of the one replay of the whole trace at the same positions"""
    c = make()
    wl = c.spec.wl
    mk = lambda: ow.oracle(c.spec, c.big, c.n_slots)  # noqa: E731
    want, _ = ow.expected(c.tag, mk, c.passes)
    counts = c.counts()
    for i in c.shards:
        sub = ss.sub_expected((c.tag, c.H, i), mk, c.own(i))
        for k, p in enumerate(c.plans):
            assert sub.replies[k].tobytes() == want[k][p.idx[i][p.own[i]]].tobytes(), (i, k)
        keyed, own, foreign = counts[i]
        assert keyed + foreign > 0, ("a shard that is sent nothing", i)
        if cid[0] == "cold":
            placed = cid[3] != "edge" or i in {r for _, r in ow.edge_places(c.sizes, c.H)}  # (a shard without a top bucket has no edge)
            assert (keyed > 0 or not placed) and (foreign > 0 or cid[3] == "edge"), (i, counts[i])
    assert sum(f for _, _, f in counts.values()) > 0
    for k, p in enumerate(c.plans):
        sent = np.zeros(len(c.passes[k]), np.int64)
        for i in c.shards:
            assert (np.diff(p.idx[i]) > 0).all()  # trace order
            sent[p.idx[i][p.own[i]]] += 1
            assert ss.keyed(wl, c.passes[k][p.idx[i][~p.own[i]]]).all()  # what is sent astray is keyed: counted as foreign, nothing else
        assert (sent[np.isin(p.home, c.shards)] == 1).all() and (sent[~np.isin(p.home, c.shards)] == 0).all()
    if c.hot_shard is not None:
        keyed, own, foreign = counts[c.hot_shard]
        assert keyed > 10_000, counts
        if (cid[0] == "slot" and cid[5] == "foreign") or (cid[0] == "row" and cid[5] > 0):
            assert foreign >= own, ("foreign fillers: at least as many foreign as home requests on the hot shard", counts[c.hot_shard])
    if cid[0] == "keyless":
        kl = ss.keyless(wl, c.passes[0])
        per = np.bincount(c.plans[0].home[kl], minlength=c.H)
        assert per.min() > 100 and per.max() - per.min() <= 1, per  # dealt
    if cid[0] == "slot" and cid[-1]:
        assert all(counts[i][1] + counts[i][2] > 0 for i in c.shards) and counts[c.hot_shard][1] + counts[c.hot_shard][2] > 65_536
    print(f"\n{'-'.join(str(x) for x in cid)}: requests {[len(p) for p in c.passes]}, shards {len(c.shards)} of {c.H}, "
          f"(own keyed, own, foreign) per shard {counts}")
