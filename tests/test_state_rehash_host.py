"""The rehash's layout rule without a GPU (dint_amd/csrc/state_rehash.h through dint_state_rehash_place_host,
include/dint_driver.h) against a numpy form that shares no code with it -- the fasthash of tests/shard_double.py, a stable
argsort, r // 4 and r % 4, a cumsum of max(ceil(k / 4) - 1, 0) -- and the numpy expected-dump form the GPU tests
(tests/test_gpu_state_rehash.py) hold dint_state_rehash to.  Every comparison is exact."""
import numpy as np
import pytest

from dint_amd import _lib
from test_state_image_host import np_bucket

EINVAL = -1
FOREIGN = np.uint64(0xFFFFFFFFFFFFFFFF)


# ------------------------------------------------------------------------------------------------ numpy reference forms
def np_rehash(dumps, hash_size, j=0, H=1):
    """expected dump_rows of the destination (hash_size, shard j of H) from the sources' dumps in srcs order: concatenate, keep
    the rows that are home to the destination, stable argsort by its local bucket"""
    keys = np.concatenate([d[0] for d in dumps]); vers = np.concatenate([d[1] for d in dumps]); vals = np.concatenate([d[2] for d in dumps])
    g = np_bucket(keys, hash_size).astype(np.int64)
    home = g % H == j
    keys, vers, vals = keys[home], vers[home], vals[home]
    o = np.argsort(g[home] // H, kind="stable")
    return keys[o], vers[o], vals[o]


def np_foreign(dumps, hash_size, j=0, H=1):
    keys = np.concatenate([d[0] for d in dumps])
    return int((np_bucket(keys, hash_size).astype(np.int64) % H != j).sum())


def np_place(keys, hash_size, j=0, H=1):
    """per row {local bucket or FOREIGN, link, slot} and the overflow need, keys in source order"""
    keys = np.asarray(keys, np.uint64)
    n, n_local = len(keys), (hash_size + H - 1) // H
    g = np_bucket(keys, hash_size).astype(np.int64)
    home = g % H == j
    bucket = np.where(home, g // H, -1)
    idx = np.nonzero(home)[0]
    o = idx[np.argsort(bucket[idx], kind="stable")]  # the home rows by bucket, source order inside a bucket
    sb = bucket[o]
    r = np.arange(len(o)) - np.searchsorted(sb, sb, side="left")  # row number inside its bucket
    k = np.bincount(sb, minlength=n_local)
    ovf = np.maximum(-(-k // 4) - 1, 0)
    base = np.cumsum(ovf) - ovf
    link = np.zeros(n, np.int64); slot = np.zeros(n, np.int64)
    link[o] = np.where(r < 4, 1, 2 + base[sb] + r // 4 - 1)
    slot[o] = r % 4
    out_b = np.where(home, bucket, 0).astype(np.uint64)
    out_b[~home] = FOREIGN
    return out_b, link.astype(np.uint32), slot.astype(np.uint32), int(ovf.sum())


def place_host(keys, hash_size, j=0, H=1):
    keys = np.ascontiguousarray(keys, "<u8")
    n = len(keys)
    b = np.zeros(max(n, 1), "<u8"); link = np.zeros(max(n, 1), "<u4"); slot = np.zeros(max(n, 1), "<u4")
    need = _lib.load().dint_state_rehash_place_host(keys.ctypes.data, n, hash_size, j, H, b.ctypes.data, link.ctypes.data, slot.ctypes.data)
    return b[:n], link[:n], slot[:n], need


def _same(keys, hash_size, j=0, H=1):
    got, want = place_host(keys, hash_size, j, H), np_place(keys, hash_size, j, H)
    for x, y in zip(got[:3], want[:3]):
        assert x.tobytes() == y.tobytes()
    assert got[3] == want[3]
    return got


def _keys_by_bucket(hash_size, counts, seed=1):
    """distinct keys, counts[b] of them in global bucket b of hash_size, shuffled"""
    rng = np.random.default_rng(seed)
    pool = rng.integers(1, 1 << 48, 400 * max(1, sum(counts)) + 4000, dtype=np.uint64)
    pool = np.unique(pool)
    rng.shuffle(pool)
    b = np_bucket(pool, hash_size).astype(np.int64)
    out = []
    for g, c in enumerate(counts):
        mine = pool[b == g]
        assert len(mine) >= c
        out.append(mine[:c])
    keys = np.concatenate(out)
    rng.shuffle(keys)
    return keys


# ------------------------------------------------------------------------------------------------ the rule
def test_entry_edges_0_1_4_5_8_9_rows():
    counts = [0, 1, 4, 5, 8, 9, 3, 0, 12, 13]
    keys = _keys_by_bucket(len(counts), counts)
    b, link, slot, need = _same(keys, len(counts))
    assert need == sum(max(-(-c // 4) - 1, 0) for c in counts) == 0 + 0 + 0 + 1 + 1 + 2 + 0 + 0 + 2 + 3
    for g, c in enumerate(counts):
        m = b == g
        assert m.sum() == c
        # no holes: slots 0 .. 3 of the inline entry, then of each overflow entry in ascending pool order
        order = np.lexsort((slot[m], link[m]))
        assert (slot[m][order] == np.arange(c) % 4).all()
        assert (link[m] == 1).sum() == min(c, 4)
        ov = np.unique(link[m][link[m] >= 2])
        assert len(ov) == max(-(-c // 4) - 1, 0) and (np.diff(ov) == 1).all()  # one contiguous run of the pool per bucket
    # the runs lie end to end in bucket order, from pool entry 0
    first = [int(link[(b == g) & (link >= 2)].min()) for g, c in enumerate(counts) if c > 4]
    assert first == sorted(first) and first[0] == 2


def test_source_order_is_kept_inside_a_bucket():
    keys = _keys_by_bucket(3, [11, 7, 9], seed=5)
    b, link, slot, _ = _same(keys, 3)
    for g in range(3):
        i = np.nonzero(b == g)[0]  # ascending source order
        pos = link[i].astype(np.int64) * 4 + slot[i]
        assert (np.diff(pos) > 0).all()


def test_one_bucket_takes_everything():
    keys = _keys_by_bucket(7, [0, 0, 0, 41, 0, 0, 0], seed=2)
    b, link, slot, need = _same(keys, 7)
    assert (b == 3).all() and need == 10 and link.max() == 2 + 9
    assert (link[:4] == 1).all() and (slot[:8] == [0, 1, 2, 3, 0, 1, 2, 3]).all() and (link[4:8] == 2).all()


def test_destination_hash_size_of_one():
    keys = np.arange(1, 23, dtype=np.uint64) * np.uint64(7919)
    b, link, slot, need = _same(keys, 1)
    assert (b == 0).all() and need == 5
    assert (slot == np.arange(22) % 4).all() and (link == np.where(np.arange(22) < 4, 1, 2 + np.arange(22) // 4 - 1)).all()


def test_shard_two_of_three_marks_foreign_rows():
    rng = np.random.default_rng(3)
    keys = np.unique(rng.integers(1, 1 << 48, 3000, dtype=np.uint64))
    rng.shuffle(keys)
    hs = 50  # 17 local buckets, about 60 rows each on this shard: long chains
    b, link, slot, need = _same(keys, hs, 2, 3)
    g = np_bucket(keys, hs).astype(np.int64)
    foreign = g % 3 != 2
    assert foreign.any() and (~foreign).any()
    assert (b[foreign] == FOREIGN).all() and (link[foreign] == 0).all() and (slot[foreign] == 0).all()
    assert (b[~foreign] == (g[~foreign] // 3).astype(np.uint64)).all() and (link[~foreign] >= 1).all()
    k = np.bincount(g[~foreign] // 3, minlength=17)
    assert need == int(np.maximum(-(-k // 4) - 1, 0).sum()) > 0
    for j in range(3):  # every shard of the layout
        _same(keys, hs, j, 3)
    assert sum(int((place_host(keys, hs, j, 3)[0] != FOREIGN).sum()) for j in range(3)) == len(keys)  # every row lands once


def test_duplicate_keys_keep_their_order():
    base = _keys_by_bucket(4, [6, 9, 2, 5], seed=7)
    keys = np.concatenate([base, base[::2], base[:5]])  # second and third copies, later in source order
    b, link, slot, _ = _same(keys, 4)
    pos = link.astype(np.int64) * 4 + slot
    for key in np.unique(keys):
        i = np.nonzero(keys == key)[0]
        assert len(set(b[i].tolist())) == 1 and (np.diff(pos[i]) > 0).all()  # the first copy stays the visible one


def test_overflow_need_is_returned_and_empty_input_is_fine():
    assert place_host(np.zeros(0, "<u8"), 10)[3] == 0
    keys = _keys_by_bucket(2, [4, 4])
    assert _same(keys, 2)[3] == 0  # four rows a bucket: inline entries only
    keys = _keys_by_bucket(2, [5, 4])
    assert _same(keys, 2)[3] == 1


def test_bad_arguments_are_refused():
    k = np.arange(4, dtype="<u8")
    assert place_host(k, 0)[3] == EINVAL
    assert place_host(k, 8, 3, 3)[3] == EINVAL
    L = _lib.load()
    assert L.dint_state_rehash_place_host(None, 4, 8, 0, 1, None, None, None) == EINVAL


def test_expected_dump_helper():
    """np_rehash, the form the GPU tests import: two sources, the second's rows after the first's inside a bucket"""
    ka, kb = _keys_by_bucket(5, [3, 0, 6, 2, 1], seed=11), _keys_by_bucket(5, [2, 2, 0, 5, 1], seed=12)
    mk = lambda k, tag: (k, np.arange(len(k), dtype="<u4") + tag, np.repeat((np.arange(len(k)) + tag)[:, None], 8, 1).astype("u1"))
    a, b = mk(ka, 0), mk(kb, 100)
    for hs, j, H in ((5, 0, 1), (3, 0, 1), (11, 1, 2)):
        keys, vers, vals = np_rehash([a, b], hs, j, H)
        g = np_bucket(keys, hs).astype(np.int64)
        assert (g % H == j).all() and (np.diff(g // H) >= 0).all()
        assert len(keys) + np_foreign([a, b], hs, j, H) == len(ka) + len(kb)
        for l in np.unique(g // H):
            v = vers[g // H == l]
            assert (np.diff(v[v < 100]) > 0).all() and (np.diff(v[v >= 100]) > 0).all()  # each source's order kept
            assert (np.nonzero(v >= 100)[0] > np.nonzero(v < 100)[0].max(initial=-1)).all()  # source 0 first
        # ... and the host rule places the concatenated keys exactly there: dump order = (bucket, link, slot) order
        bk, link, slot, _ = place_host(np.concatenate([ka, kb]), hs, j, H)
        home = bk != FOREIGN
        o = np.lexsort((slot[home], link[home], bk[home]))
        assert np.concatenate([ka, kb])[home][o].tobytes() == keys.tobytes()
