"""Host checks of the tooling behind tests/test_gpu_kv_collide.py: the key searches of tests/kvkeys.py against the oracle's own
fasthash64, tracegen.tatp_random unchanged for its earlier callers, and for every trace of tests/kv_collide.py the conditions
that make its case mean something -- computed from the requests and the oracle alone.  A seed that misses a condition is
replaced; the condition stays."""
import hashlib
import struct

import numpy as np
import pytest

import kv_collide as kc
import kvkeys
import tracegen
from dint_amd import wire
from oracle import oracle as orc

W = wire.Workload


def sig(key, hs):
    """(bucket, quadrant, key hash) through the oracle's hash, not through kvkeys"""
    h = orc.fasthash64(struct.pack("<Q", int(key)))
    return h % hs, (h % (4 * hs)) // hs, (h >> 40) & 511


def hash_size(case, table):
    if case.wl == W.STORE:
        return kc.STORE_HS
    return kc.tatp_base()[1][table] if case.wl == W.TATP else kc.sb_hs(case.engine["n_rows"])


def test_key_sig_is_the_oracles_hash():
    rng = np.random.default_rng(1)
    keys = np.concatenate([np.array([0, 1, 7, 2**64 - 1, 2**63, 1 << 40, 1 << 48, 511 << 40, 0xFFFF << 48, 7 | (1 << 32)], np.uint64),
                           rng.integers(0, 2**63, 150, dtype=np.uint64) * np.uint64(2) + np.uint64(1), np.uint64(1) << rng.integers(32, 64, 40).astype(np.uint64),
                           rng.integers(0, 3000, 100, dtype=np.uint64)])
    for hs in (1125, 4218, 22_500, 75_000, 1):
        b, q, k = kvkeys.key_sig(keys, hs)
        want = np.array([sig(x, hs) for x in keys.tolist()], np.uint64)
        assert (b == want[:, 0]).all() and (q == want[:, 1]).all() and (k == want[:, 2]).all(), hs
        assert (kvkeys.np_bucket(keys, hs) == b).all()


LIKE = [(key, hs, key_of, kh, q) for key, hs, key_of in ((7, 1125, None), (7 | (1 << 32), 4218, kvkeys.cf_key_of), (7, 750, None))
        for kh in (False, True) for q in (False, True)] + [(kc.STORE_HOT, kc.STORE_HS, None, kh, None) for kh in (False, True)]  # (the store has no quadrants)


@pytest.mark.parametrize("key,hs,key_of,same_kh,same_quadrant", LIKE)
def test_keys_like_gives_the_relation_asked_for(key, hs, key_of, same_kh, same_quadrant):
    n = 2 if not same_kh else 1
    got = kvkeys.keys_like(key, hs, n, same_kh=same_kh, same_quadrant=same_quadrant, seed=11, key_of=key_of, exclude=(12345,))
    assert len(got) == n == len(set(got.tolist())) and int(key) not in got.tolist() and 12345 not in got.tolist()
    b0, q0, k0 = sig(key, hs)
    for x in got.tolist():
        b, q, k = sig(x, hs)
        assert b == b0 and (k == k0) == same_kh and (same_quadrant is None or (q == q0) == same_quadrant), (x, b, q, k)
        if key_of is not None:
            assert 1 <= (x >> 32) & 0xFF <= 4 and (x >> 40) in (0, 8, 16)  # a well-formed CALL_FORWARDING key
    again = kvkeys.keys_like(key, hs, n, same_kh=same_kh, same_quadrant=same_quadrant, seed=11, key_of=key_of, exclude=(12345,))
    assert (again == got).all()


@pytest.mark.parametrize("hs,n_groups,per,key_of", [(1125, 8, 3, None), (2812, 8, 3, kc.sf_key_of), (4218, 8, 3, kvkeys.cf_key_of), (kc.STORE_HS, 8, 3, None),
                                                     (75_000, 4, 3, None), (75_000, 8, 2, "accounts")])
def test_collision_groups_share_bucket_and_key_hash(hs, n_groups, per, key_of):
    if key_of == "accounts":
        g = kc.sb_chunks().pairs[0:8]
        g = np.array([x[1] for x in g], np.uint64)
        assert (g < kc.SB_ACCT).all()  # populated accounts
    else:
        g = kvkeys.collision_groups(hs, n_groups, per, seed=5, key_of=key_of)
    assert g.shape == (n_groups, per) and len(set(g.ravel().tolist())) == n_groups * per
    buckets = set()
    for row in g.tolist():
        s = [sig(x, hs) for x in row]
        assert len({(b, k) for b, _, k in s}) == 1, row
        buckets.add(s[0][0])
    assert len(buckets) == n_groups


def test_colliding_pairs_of_a_populated_table():
    hs = kc.sb_hs(kc.SB_ACCT)
    for same in (False, True):
        p = kvkeys.colliding_pairs(np.arange(kc.SB_ACCT, dtype=np.uint64), hs, same)
        assert len(p) > 50
        for a, b in p[:20].tolist():
            sa, sb = sig(a, hs), sig(b, hs)
            assert a != b and sa[0] == sb[0] and sa[2] == sb[2] and (sa[1] == sb[1]) == same


TATP_RANDOM_DIGESTS = [  # sha256 of tatp_random's bytes as of the commit before `pools` came, over TatpOracle(2000, populate_n=40)'s rows
    (dict(n=1, seed=0, n_sub_touch=40, well_formed=True), "894a4a1a95ef7c33332af5c7b4557f0aae79877f32b1198586e2a2ffab16f651"),
    (dict(n=4096, seed=4136, n_sub_touch=40, well_formed=True), "87b557e32a93c28f133a9ed7b232477e4183bb5ec1c9119fd37823a52de0e65c"),
    (dict(n=3000, seed=9, n_sub_touch=6, well_formed=False), "b19045bf5ec985ee717b8a58562d799f18ca9939730b47b7436bd47977724a63"),
    (dict(n=2500, seed=77, n_sub_touch=400, well_formed=True), "1dda4f960ddfa78266d20c85d9c5f4448f665cb7815039d8e730d9207ae7dead"),
]


def test_tatp_random_without_pools_is_unchanged_and_pools_are_used():
    o = orc.TatpOracle(2000, log_entries=16, populate_n=40)
    ex = [o.dump(t)[0] for t in range(5)]
    for kw, digest in TATP_RANDOM_DIGESTS:
        kw = dict(kw)
        assert hashlib.sha256(tracegen.tatp_random(kw.pop("n"), ex, **kw).tobytes()).hexdigest() == digest, kw
    pools = [[5, 9], [6], [1 | (1 << 32)], [2 | (2 << 32), 3 | (1 << 32)], [7 | (1 << 32) | (8 << 40)]]
    m = tracegen.tatp_random(500, ex, seed=3, pools=pools)
    for t in range(5):
        assert set(m["key"][m["table"] == t].tolist()) == set(pools[t])


# ---- the traces of the GPU tests ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(kc.CASES))
def test_trace_holds_what_its_case_is_about(name):
    c = kc.CASES[name]()
    assert c is kc.CASES[name]()  # built once
    assert max(len(p) for p in c.passes) <= 40_000
    known = {W.STORE: (0, 1, 2), W.TATP: (0, 1, 2, 12, 13, 14, 18, 19, 22, 23, 24), W.SMALLBANK: (0, 1, 2, 3, 4, 5, 6)}[c.wl]
    assert all(np.isin(p["type"], known).all() for p in c.passes)  # no unknown type: bad_requests stays 0
    fresh = c.oracle()
    dump0 = [fresh.dump()] if c.wl == W.STORE else [fresh.dump(t) for t in range(len(c.rows))]
    for table, keys, passes in c.pairs:
        hs = hash_size(c, table)
        s = [sig(k, hs) for k in keys]
        assert len(set(keys)) == len(keys) and len({(b, kh) for b, _, kh in s}) == 1, (name, keys, s)
        for k in passes:
            assert all(kc.count(c, k, table, key) > 0 for key in keys), (name, k)
    for table, key, passes in c.cold:
        for k in passes:
            assert 1 <= kc.count(c, k, table, key) <= 8, (name, k, kc.count(c, k, table, key))
    for table, key, at_least in c.hot:
        hs = hash_size(c, table)
        for k, n in at_least.items():
            # (a big sub everywhere but in c-0.02, dominant_key's second mix: a hot CALL_FORWARDING row of a dozen to 280 requests)
            assert (n >= 100 or name.startswith("c-0.02")) and kc.count(c, k, table, key) >= n, (name, k, n, kc.count(c, k, table, key))
        # the hot row's bucket holds no duplicate row, and nothing but the named keys is requested in it
        b0 = sig(key, hs)[0]
        dk = dump0[table][0]
        in_b = dk[kvkeys.np_bucket(dk, hs) == np.uint64(b0)]
        assert len(in_b) == len(set(in_b.tolist())), (name, in_b)
        named = {key} | {x for t2, ks, _ in c.pairs if t2 == table for x in ks} | (set(c.control[1:]) if c.control else set())
        for p in c.passes:
            sel = kvkeys.np_bucket(p["key"], hs) == np.uint64(b0)
            if c.wl != W.STORE:
                sel &= p["table"] == table
            assert set(p["key"][sel].tolist()) <= named, name
    if c.control:
        table, h, n2 = c.control
        sh, sn = sig(h, hash_size(c, table)), sig(n2, hash_size(c, table))
        assert sh[0] == sn[0] and sh[1] != sn[1] and sh[2] != sn[2]
        assert all(kc.count(c, k, table, n2) > 0 for k in range(1, len(c.passes) - 1))
    if name[0] in "bce":  # the last pass is the hot key's alone: back in closed form
        table, keys, _ = c.pairs[0] if c.pairs else (c.control[0], list(c.control[1:]), None)
        assert kc.count(c, len(c.passes) - 1, table, keys[1]) == 0 and kc.count(c, len(c.passes) - 1, table, keys[0]) > (0 if name.startswith("c-0.02") else 100)
    if name.startswith("a-"):  # cold throughout: a key at most 20 requests, a bucket at most 64 records; colliding keys meet in every pass
        for k, p in enumerate(c.passes):
            met = 0
            for table, keys, _ in c.pairs:
                n = [kc.count(c, k, table, key) for key in keys]
                assert max(n) <= 20, (name, k, n)
                hs = hash_size(c, table)
                sel = kvkeys.np_bucket(p["key"], hs) == np.uint64(sig(keys[0], hs)[0])
                if c.wl != W.STORE:
                    sel &= p["table"] == table
                assert sel.sum() <= 64, (name, k, int(sel.sum()))
                met += sum(x > 0 for x in n) >= 2
            assert met >= (len(c.pairs) if k == len(c.passes) - 1 else 8), (name, k, met, len(c.pairs))
    if name == "a-store":  # some keys are inserted by the trace and then read; one of every group never exists
        allp = np.concatenate(c.passes)
        for _, keys, _ in c.pairs:
            assert not (allp["type"][allp["key"] == np.uint64(keys[2])] == 2).any()
            for key in keys[:2]:
                at = np.nonzero(allp["key"] == np.uint64(key))[0]
                ins = at[allp["type"][at] == 2]
                assert len(ins) == 1 and (allp["type"][at[at > ins[0]]] == 0).any(), key
    if name == "a-tatp":  # well formed, all eleven op types, INSERTs and DELETEs of colliding keys
        allp = np.concatenate(c.passes)
        assert c.errors == 0 and set(allp["type"].tolist()) == {0, 1, 2, 12, 13, 14, 18, 19, 22, 23, 24}
        grp = np.isin(allp["key"], np.array([x for _, ks, _ in c.pairs for x in ks], np.uint64))
        assert (np.isin(allp["type"][grp], (18, 19)).sum() > 40) and (np.isin(allp["type"][grp], (22, 23)).sum() > 40)
    if name == "a-smallbank":
        allp = np.concatenate(c.passes)
        grp = np.isin(allp["key"], np.array([x for _, ks, _ in c.pairs for x in ks], np.uint64))
        assert set(allp["type"][grp].tolist()) == set(range(7)) and set(allp["table"][grp].tolist()) == {0, 1}
    if name.startswith("f-") and "no-account" not in name:
        assert all(x < c.populate for x in c.pairs[0][1]) and c.errors == 0  # both accounts are populated
    if name.startswith("f-no-account") or name.startswith("e-missing"):
        n_key = c.pairs[0][1][1]
        assert n_key not in dump0[0][0].tolist() and n_key not in c.rows[0][0].tolist()
