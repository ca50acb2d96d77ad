"""A server's table occupancy and chain shape reported from the GPU (include/dint_abi.h dint_state_stats,
dint_amd/csrc/k_stats.hip, dint_amd/recovery.py table_stats / check_tables / rehash_advice).  Every fixture is checked four ways
against each other -- the device report, the host form over the engine's downloaded own image, the numpy form over the same
bytes (tests/test_state_stats_host.py np_image_stats) and the identities every report satisfies -- and against forms that use
neither the image nor the rule: dump_rows with the fasthash of tests/shard_double.py, export's count, read_locks.  Every
comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import tracegen
from dint_amd import _lib, recovery, wire
from test_gpu_state_rehash import _delete_rows, _same_bucket_keys, _store_insert, _vals, chained  # noqa: F401  (chained: a fixture)
from test_state_image_host import np_bucket, same_dump
from test_state_stats_host import NO_BUCKET, assert_identities, host_stats, np_image_stats

W, T, S = wire.Workload, wire.Tatp, wire.Sb
EINVAL, ESTATE = -1, -5
NTAB = {W.STORE: 1, W.TATP: 5, W.SMALLBANK: 2}
pytestmark = pytest.mark.gpu


def _engine(*a, **kw):
    from dint_amd.engine import Engine

    return Engine(*a, **kw)


def _hist(values, bins):
    return np.bincount(np.minimum(np.asarray(values, np.int64), bins - 1), minlength=bins).tolist()


def _locks_words(e, t):
    if e.workload == W.STORE:
        return 0
    a, b = e.read_locks(t)
    return int(((a != 0) | (b != 0)).sum())


def _check(e, long_bucket=False):
    """the device report of every table of `e` against the host form and the numpy form over its own image, the identities,
    dump_rows, export's count and read_locks; returns the device report"""
    dev = e.state_stats()
    buf, n, ist = e.state_export(e.shard_index, e.shard_count)
    img = buf[:n].cpu().numpy()
    rc, host = host_stats(img)
    want = np_image_stats(img)
    assert rc == len(dev) == len(want) == NTAB[e.workload]
    for t, d in enumerate(dev):
        if not long_bucket:
            assert d["buckets_unchecked"] == 0  # first: the cap must not hide a wrong shadowed_rows
        print(e.workload.name, t, {k: v for k, v in d.items() if not k.endswith("_hist")})
        assert host[t] == want[t], (t, {k: (host[t][k], want[t][k]) for k in want[t] if host[t][k] != want[t][k]})
        no_pool = dict(d, pool_cap=0, pool_top=0)
        assert no_pool == host[t], (t, {k: (no_pool[k], host[t][k]) for k in no_pool if no_pool[k] != host[t][k]})
        assert_identities(d)
        assert d["overflow_entries"] <= d["pool_top"] <= d["pool_cap"]
        keys = e.dump_rows(t)[0]
        assert d["rows"] == len(keys)
        local = np_bucket(keys, e.hash_size(t)).astype(np.int64) // e.shard_count
        per_bucket = np.bincount(local, minlength=d["buckets"])
        assert len(per_bucket) == d["buckets"] and d["rows_hist"] == _hist(per_bucket, 33) and d["most_rows"] == int(per_bucket.max(initial=0))
        if not long_bucket:
            assert d["shadowed_rows"] == len(keys) - len(np.unique(keys))
        assert d["locks_held"] == _locks_words(e, t)
    assert sum(d["overflow_entries"] for d in dev) == ist["overflow_entries"] and sum(d["rows"] for d in dev) == ist["rows"]
    return dev


def _load(e, keys, tag=1, table=0):
    keys = np.asarray(keys, np.uint64)
    e.load_rows(table, keys, np.arange(len(keys), dtype="<u4"), _vals(keys, tag))


# ---------------------------------------------------------------------------------------------- 1. a blank engine stays blank
def test_a_blank_engine_reports_zeros_and_stays_blank():
    src = _engine(W.STORE, n_rows=64)
    src.populate(20)
    for into in ("rehash", "import"):
        e = _engine(W.STORE, n_rows=64)
        (d,) = e.state_stats()
        assert d["buckets"] == d["buckets_empty"] == d["chain_hist"][0] == d["rows_hist"][0] == 288
        assert d["longest_chain_bucket"] == NO_BUCKET and d["pool_cap"] == 288 // 4 + 4096
        zero = dict(d, buckets=0, buckets_empty=0, longest_chain_bucket=0, pool_cap=0)
        zero["chain_hist"][0] = zero["rows_hist"][0] = 0
        assert all(v == 0 or v == [0] * len(v) for v in zero.values()), zero
        _check(e)
        if into == "rehash":
            assert e.state_rehash([src])["rows_placed"] == 240
        else:
            buf, n, _ = src.state_export(0, 1)
            assert e.state_import(buf, n)["rows"] == 240
        assert e.state_digest() == src.state_digest()
        assert _check(e)[0]["rows"] == 240
        e.close()
    src.close()


# ---------------------------------------------------------------------------------------------- 2. churn
def test_store_churn_holes_recycled_entries_and_inline_entries_anywhere(chained):  # noqa: F811
    e = chained
    (d,) = _check(e)
    assert d["buckets"] == 288  # more than one workgroup, no multiple of 256
    assert d["inline_unlinked"] + (d["buckets"] - d["inline_first"]) > 0 and d["holes"] > 0  # or the case is void
    ck = recovery.check_tables(e)
    assert ck["ok"] and ck["tables"][0]["rows"] == ck["tables"][0]["digest_rows"] == d["rows"]


# ---------------------------------------------------------------------------------------------- 3. long chains, both overflow bins
def test_store_long_chains_fill_the_histograms_to_their_last_bins():
    e = _engine(W.STORE, n_rows=16, pool_entries=4096)
    assert e.hash_size(0) == 72
    rng = np.random.default_rng(3)
    keys = tracegen.store_key(rng.permutation(1000)[:960, None], np.arange(1, 4)[None, :], 0).ravel()
    rng.shuffle(keys)
    _load(e, keys)
    _load(e, _same_bucket_keys(72, 11, 40, 50_000_000), 2)  # one bucket past 16 entries and 32 rows
    (d,) = _check(e)
    assert d["rows"] == 2920 and d["longest_chain"] >= 17 and d["most_rows"] >= 33
    assert d["chain_hist"][16] >= 1 and d["rows_hist"][32] >= 1 and sum(d["chain_hist"][8:16]) > 30 and d["longest_chain_bucket"] == 11
    e.close()


# ---------------------------------------------------------------------------------------------- 4. a bucket past the comparison's cap
def test_a_bucket_of_more_than_64_entries_is_counted_but_not_compared():
    e = _engine(W.STORE, n_rows=16, pool_entries=1024)
    long_keys = _same_bucket_keys(72, 7, 270, 60_000_000)
    _load(e, long_keys)
    _load(e, long_keys[100:101], 2)  # one key twice inside the long bucket
    other = _same_bucket_keys(72, 8, 6, 70_000_000)
    _load(e, np.concatenate([other, other[:2]]), 3)  # ... and two in a bucket that is compared
    (d,) = _check(e, long_bucket=True)
    assert d["buckets_unchecked"] == 1 and d["longest_chain"] == 68 and d["longest_chain_bucket"] == 7 and d["most_rows"] == 271
    keys = e.dump_rows(0)[0]
    assert len(keys) - len(np.unique(keys)) == 3 and d["shadowed_rows"] == 2  # the long bucket's duplicate is not counted
    e.close()


# ---------------------------------------------------------------------------------------------- 5. duplicates
def test_shadowed_rows_within_one_entry_and_across_entries():
    e = _engine(W.STORE, n_rows=64, pool_entries=1024)
    a, b = _same_bucket_keys(288, 5, 2, 10_000_000)
    _load(e, [a, b]); _load(e, [a], 2)                       # bucket 5: [a b a'] in one entry
    k = _same_bucket_keys(288, 9, 6, 20_000_000)
    _load(e, k[:4])                                          # bucket 9: the inline entry full ...
    _store_insert(e, k[:1], 4)                               # ... an INSERT of an existing key opens a newer entry: [k0'] -> [k0 k1 k2 k3]
    _load(e, [k[4], k[4], k[5], k[1]], 5)                    # [k0' k4 k4' k5] and [k1'] in a third
    rng = np.random.default_rng(8)
    fill = tracegen.store_key(rng.permutation(500), 2, 0)
    fill = fill[~np.isin(np_bucket(fill, 288).astype(np.int64), (5, 9))]
    twice = np.concatenate([fill, fill, fill[::3]])
    _load(e, twice[rng.permutation(len(twice))], 6)
    (d,) = _check(e)
    in9 = e.dump_rows(0)[0][np_bucket(e.dump_rows(0)[0], 288).astype(np.int64) == 9]
    assert in9.tolist() == [k[1], k[0], k[4], k[4], k[5], k[0], k[1], k[2], k[3]]  # chain order as built
    assert d["shadowed_rows"] == 1 + 3 + len(fill) + len(fill[::3])
    e.close()


# ---------------------------------------------------------------------------------------------- 6. more buckets than one sweep of the grid
def test_a_table_larger_than_one_sweep_of_the_grid():
    e = _engine(W.STORE, n_rows=120_000, pool_entries=4096)
    assert e.hash_size(0) == 540_000 > 2048 * 256  # DINT_STATE_STATS_GRID workgroups of 256 buckets
    keys = tracegen.store_key(np.arange(30_000), 1, 0)
    _load(e, np.concatenate([keys, keys[:500]]))
    (d,) = e.state_stats()
    assert d["buckets_unchecked"] == 0
    assert_identities(d)
    dump = e.dump_rows(0)[0]
    per_bucket = np.bincount(np_bucket(dump, 540_000).astype(np.int64), minlength=540_000)
    assert d["buckets"] == 540_000 and d["rows"] == len(dump) == 30_500 and d["shadowed_rows"] == 500
    assert d["rows_hist"] == _hist(per_bucket, 33) and d["buckets_empty"] == int((per_bucket == 0).sum())
    ent = -(-per_bucket // 4)  # (rows loaded into a fresh table: every chain compact)
    assert d["chain_hist"] == _hist(ent, 17) and d["entries"] == int(ent.sum()) and d["overflow_entries"] == int(np.maximum(ent - 1, 0).sum())
    assert d["longest_chain"] == int(ent.max()) and d["longest_chain_bucket"] == int(np.argmax(ent)) and d["most_rows"] == int(per_bucket.max())
    far = np.flatnonzero(per_bucket)[-1]
    assert far >= 2048 * 256  # rows behind the first sweep were seen
    e.close()


# ---------------------------------------------------------------------------------------------- 7. tatp and smallbank
@pytest.fixture(scope="module", params=[0, _lib.FLAG_LOCK_SAME_KEY])
def tatp(request):
    e = _engine(W.TATP, n_rows=2000, log_entries=1 << 16, flags=request.param)
    e.populate(2000)
    existing = [e.dump_rows(t)[0] for t in range(5)]
    few = [ks[ks % np.uint64(1 << 32) < 40] for ks in existing]
    e.submit(tracegen.tatp_random(4000, few, seed=13, n_sub_touch=40))
    m = np.zeros(1500, wire.TATP_MSG)  # and locks all over the tables
    rng = np.random.default_rng(2)
    m["type"], m["table"] = T.ACQUIRE_LOCK, rng.integers(0, 5, 1500)
    m["key"] = [existing[t][i % len(existing[t])] for t, i in zip(m["table"], rng.integers(0, 1 << 30, 1500))]
    assert (e.submit(m)["type"] == T.GRANT_LOCK).sum() > 500
    yield e
    e.close()


def test_tatp_five_tables_of_three_sizes_with_lock_bytes(tatp):
    dev = _check(tatp)
    assert [d["buckets"] for d in dev] == [750, 750, 1875, 1875, 2812]
    assert all(d["locks_held"] > 50 for d in dev) and sum(d["overflow_entries"] for d in dev) > 0
    assert recovery.check_tables(tatp)["ok"]


def test_smallbank_128_byte_entries_with_counters_held():
    e = _engine(W.SMALLBANK, n_rows=2000, log_entries=1 << 16)
    e.populate(2000)
    e.submit(tracegen.sb_random(4000, seed=9, n_acct_touch=300))
    dev = _check(e)
    assert [d["buckets"] for d in dev] == [750, 750] and [d["rows"] for d in dev] == [2000, 2000]
    assert all(d["locks_held"] > 0 for d in dev)
    e.close()


# ---------------------------------------------------------------------------------------------- 8. a sharded set
def test_three_shards_add_up_and_name_global_buckets():
    G = 3
    shards = [_engine(W.STORE, n_rows=64, shard_index=s, shard_count=G, pool_entries=2048) for s in range(G)]
    rng = np.random.default_rng(12)
    keys = tracegen.store_key(rng.permutation(700)[:, None], np.arange(1, 4)[None, :], 0).ravel()
    twice = keys[::9]  # 234 keys loaded a second time
    keys = np.concatenate([keys, twice])
    rng.shuffle(keys)
    for e in shards:
        _load(e, keys)  # (a shard keeps the rows that are home to it)
    per = [_check(e)[0] for e in shards]
    (tot,) = recovery.table_stats(shards)
    dump = np.concatenate([e.dump_rows(0)[0] for e in shards])
    g = np_bucket(dump, 288).astype(np.int64)
    per_bucket = np.bincount(g, minlength=288)
    assert tot["rows"] == len(dump) == len(keys) and tot["buckets"] == 288 and tot["rows_hist"] == _hist(per_bucket, 33)
    assert tot["shadowed_rows"] == len(dump) - len(np.unique(dump)) == len(twice) == 234
    assert tot["pool_cap"] == 3 * 2048 and tot["pool_top"] == sum(p["pool_top"] for p in per) == tot["overflow_entries"]
    ent = -(-per_bucket // 4)  # (loaded, never deleted: every chain compact)
    assert tot["longest_chain"] == int(ent.max()) == max(p["longest_chain"] for p in per)
    assert tot["longest_chain_bucket"] == int(np.argmax(ent))  # the lowest global id that attains it
    assert tot["most_rows"] == int(per_bucket.max())
    for s, p in enumerate(per):
        assert p["longest_chain_bucket"] % G == s and ent[p["longest_chain_bucket"]] == p["longest_chain"]
    assert_identities(tot)
    for e in shards:
        e.close()


# ---------------------------------------------------------------------------------------------- 9. the loop closed
def test_advice_then_rehash_gives_the_closed_form_and_no_more_advice():
    src = _engine(W.STORE, n_rows=64, pool_entries=4096)
    rng = np.random.default_rng(21)
    keys = tracegen.store_key(rng.permutation(960)[:, None], np.arange(1, 4)[None, :], 0).ravel()  # 10 rows a bucket, no key twice
    rng.shuffle(keys)
    _load(src, keys)
    adv = recovery.rehash_advice([src])
    assert adv["needed"] and adv["load"] == [2880 / 288] and adv["locks_held"] == 0
    n_new = adv["n_rows"]
    assert n_new == recovery.advise_n_rows(W.STORE, [2880]) and recovery.hash_sizes(W.STORE, n_new)[0] * 8 >= 2880 * 3
    H = 2
    dst = [_engine(W.STORE, n_rows=n_new, shard_index=j, shard_count=H, pool_entries=4096) for j in range(H)]
    assert [e.hash_size(0) for e in dst] == recovery.hash_sizes(W.STORE, n_new) * H
    recovery.rehash([src], dst)
    for e in dst:
        _check(e)
    (got,) = recovery.table_stats(dst)
    hs = dst[0].hash_size(0)
    k = np.bincount(np_bucket(keys, hs).astype(np.int64), minlength=hs)  # from the source's keys alone
    ent = -(-k // 4)
    assert got["rows"] == 2880 and got["entries"] == int(ent.sum()) and got["holes"] == int((4 * ent - k).sum())
    assert got["inline_first"] == got["buckets"] - got["buckets_empty"] == int((k > 0).sum()) and got["inline_unlinked"] == 0
    assert got["overflow_entries"] == int(np.maximum(ent - 1, 0).sum()) == got["pool_top"]
    assert got["hit_entries"] == int(sum((np.arange(x) // 4 + 1).sum() for x in k))
    assert got["chain_hist"] == _hist(ent, 17) and got["rows_hist"] == _hist(k, 33) and got["shadowed_rows"] == 0
    after = recovery.rehash_advice(dst)
    assert not after["needed"] and after["load"][0] <= 8 / 3 and after["n_rows"] == n_new
    for e in [src] + dst:
        e.close()


# ---------------------------------------------------------------------------------------------- 10. lock words, read-only, refusals
def test_locks_held_is_what_a_refused_rehash_reports(tatp):
    held = sum(d["locks_held"] for d in tatp.state_stats())
    dst = _engine(W.TATP, n_rows=4000, log_entries=1 << 12, flags=tatp.flags)
    with pytest.raises(_lib.DintError, match=f"dint error {ESTATE}:"):
        dst.state_rehash([tatp])
    assert dst.last_rehash["locks_held"] == held > 0 and recovery.rehash_advice([tatp])["locks_held"] == held
    dst.close()


def test_a_report_changes_nothing(tatp):
    def state(e):
        return ([e.dump_rows(t) for t in range(5)], [e.read_locks(t) for t in range(5)], e.stats(), e.state_digest())

    before = state(tatp)
    first = tatp.state_stats()
    assert tatp.state_stats() == first
    after = state(tatp)
    for x, y in zip(before[0] + before[1], after[0] + after[1]):
        assert same_dump(x, y)
    assert before[2:] == after[2:]


def test_refusals():
    for e in (_engine(W.FASST, n_slots=1000), _engine(W.TPL, n_slots=1000), _engine(W.LOG, log_entries=1 << 10)):
        with pytest.raises(_lib.DintError, match=f"dint error {ESTATE}:"):
            e.state_stats()
        e.close()
    e = _engine(W.TATP, n_rows=100)
    out = (_lib.TableStats * 5)()
    assert e._L.dint_state_stats(e._h, out, 4, None) == EINVAL and b"room for" in e._L.dint_last_error()
    assert e._L.dint_state_stats(e._h, None, 5, None) == EINVAL
    assert e._L.dint_state_stats(e._h, out, 5, None) == 5 and out[4].buckets == e.hash_size(4)
    e.close()
    assert C.sizeof(_lib.TableStats) == 640
