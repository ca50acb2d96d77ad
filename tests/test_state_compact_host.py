"""The table compaction's rule without a GPU (dint_amd/csrc/state_compact.h through dint_state_compact_view_host,
include/dint_driver.h) against a numpy / Python form over a view's raw bytes, written from the rule's description and the layout
comment of dint_kv_core.h alone: it shares no code with the rule (its census is the numpy census of test_state_verify_host.py).
The verify tests' sound table in three shapes, hand-built buckets, the refusals, idempotence and dry runs, and the host build of
dint_kv_core.h driven through random churn, compacted, and driven on beside an uncompacted twin.  Every comparison is exact.

`python tests/test_state_compact_host.py FILE` writes every view below with the numpy form's return value, reports and bytes
afterwards into FILE, for the stand-alone sanitizer program tests/native/state_compact_main.cc."""
import ctypes as C
import os
import struct
import subprocess
import sys

if __name__ == "__main__":  # (run as a script: pytest's conftest is not there to put the repository on the path)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import pytest

from dint_amd import _lib, recovery, wire
from test_state_image_host import np_bucket
from test_state_verify_host import (CHANGES, KINDS, NLISTS, SHAPE, Tab, View, bent_view, host_verify, is_clean, keys_of, np_verify,
                                    np_verify_table, one_change, sound_view, truncated_view)

W = wire.Workload
EINVAL, ENOMEM, ESTATE = -1, -3, -5
DRY = 1
GATE = ("bad_chains", "cross_linked", "linked_beyond_top", "list_bad_links", "stray_valid_entries", "misplaced_rows", "odd_valid_bytes")
CFIELDS = ("rows", "entries_before", "entries_after", "overflow_before", "overflow_after", "pool_top_before", "pool_top_after",
           "holes_before", "holes_after", "buckets_rewritten", "unaccounted_dropped", "staging_bytes")
LEAKS = (0, 1, 64, 65)


def host_compact(view, flags=0, cap=5):
    out = (_lib.TableCompact * 5)()
    rc = _lib.load().dint_state_compact_view_host(C.byref(view.c_view()), out, cap, flags)
    return rc, [out[t].as_dict() for t in range(len(view.tabs))]


# ------------------------------------------------------------------------------------------------ the numpy / Python form
def _chain(t, b):
    """bucket b's chain as entry rows of t.entries, in chain order (the census has said it ends)"""
    out, link = [], t.u32(b, 56)
    while link:
        e = b if link == 1 else t.n_local + link - 2
        out.append(e)
        link = t.u32(e, 52)
    return out


def np_compact_table(t, census, val_size, dry):
    """one table whose census passed the gate: its report, and unless dry its bytes rewritten as the rule says"""
    ent, n_local, stride = t.entries, t.n_local, t.stride
    per = []  # per bucket: [(entry row, slot)] of its valid rows in chain order
    entries_before = rewritten = 0
    for b in range(n_local):
        ch = _chain(t, b)
        entries_before += len(ch)
        rows = [(e, s) for e in ch for s in range(4) if ent[e, 48 + s]]
        per.append(rows)
        k = len(rows)
        if k == 0:
            rewritten += t.u32(b, 56) != 0
        else:
            want = [[1] * 4] * ((k - 1) // 4) + [[1] * (k - 4 * ((k - 1) // 4)) + [0] * (4 * ((k - 1) // 4 + 1) - k)]
            have = [[int(x != 0) for x in ent[e, 48:52]] for e in ch]
            rewritten += not (ch[0] == b and have == want)
    counts = [max(0, (len(r) + 3) // 4 - 1) for r in per]
    new_top = sum(counts)
    n_rows = sum(len(r) for r in per)
    entries_after = sum((len(r) + 3) // 4 for r in per)
    rep = dict(rows=n_rows, entries_before=entries_before, entries_after=entries_after, overflow_before=census["linked"],
               overflow_after=new_top, pool_top_before=census["pool_top"], pool_top_after=new_top,
               holes_before=4 * entries_before - n_rows, holes_after=4 * entries_after - n_rows, buckets_rewritten=rewritten,
               unaccounted_dropped=census["unaccounted"], staging_bytes=new_top * stride)
    assert n_rows == census["rows"]
    if dry:
        return rep
    old = ent.copy()

    def put(dst, slot, src, s):
        dst[8 * slot:8 * slot + 8] = old[src, 8 * s:8 * s + 8]
        dst[32 + 4 * slot:36 + 4 * slot] = old[src, 32 + 4 * s:36 + 4 * s]
        dst[48 + slot] = 1
        dst[64 + val_size * slot:64 + val_size * (slot + 1)] = old[src, 64 + val_size * s:64 + val_size * (s + 1)]

    base = 0
    for b, rows in enumerate(per):
        k = len(rows)
        if k == 0:
            ent[b, :60] = 0  # keys, versions, valid bytes, next, head ...
            ent[b, 64:64 + 4 * val_size] = 0  # ... and the four values: unused slots like any other
            continue
        n_ent = (k + 3) // 4
        new = np.zeros((n_ent, stride), np.uint8)
        new[0] = old[b]                          # the inline entry keeps lockw, counters and owner keys ...
        new[0, :60] = 0                          # ... but keys, versions, valid bytes, next and head
        new[0, 64:64 + 4 * val_size] = 0         # ... and the four values are the rule's
        new[0, 56:60] = np.frombuffer(struct.pack("<I", 1), np.uint8)
        for r, (e, s) in enumerate(rows):
            put(new[r // 4], r % 4, e, s)
        for x in range(n_ent):
            nxt = base + x + 2 if x + 1 < n_ent else 0  # chain position x + 1 is pool entry base + x
            new[x, 52:56] = np.frombuffer(struct.pack("<I", nxt), np.uint8)
        ent[b] = new[0]
        ent[n_local + base:n_local + base + n_ent - 1] = new[1:]
        base += n_ent - 1
    assert base == new_top
    old_top = min(t.top, t.pool_cap)
    ent[n_local + new_top:n_local + max(new_top, old_top), 48:56] = 0
    t.top = new_top
    h = t.heads()
    h[:] = ((h >> np.uint64(32)) + np.uint64(1)) << np.uint64(32)
    return rep


def np_compact(view, dry=False):
    """(rc, reports); unless dry or refused the view's bytes are rewritten"""
    census = [np_verify_table(t, view.shard)[0] for t in view.tabs]
    if any(c[k] for c in census for k in GATE):
        return ESTATE, [dict({k: 0 for k in CFIELDS}, verify=c) for c in census]
    val_size = SHAPE[view.workload][2]
    return len(view.tabs), [dict(np_compact_table(t, c, val_size, dry), verify=c) for t, c in zip(view.tabs, census)]


# ------------------------------------------------------------------------------------------------ views
def dress(view, seed=1):
    """what a census does not look at, made visible: random versions and values in every slot of every entry (stale ones
    included), lock bytes, smallbank counters and owner keys in every inline entry, and stale bytes there in the overflow entries"""
    rng = np.random.default_rng(seed)
    val_size = SHAPE[view.workload][2]
    for t in view.tabs:
        n = len(t.entries)
        t.entries[:, 32:48] = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        t.entries[:, 64:64 + 4 * val_size] = rng.integers(0, 256, (n, 4 * val_size), dtype=np.uint8)
        t.entries[:, 60:64] = rng.integers(1, 256, (n, 4), dtype=np.uint8)  # lockw
        if t.stride == 128:
            t.entries[:, 96:128] = rng.integers(0, 256, (n, 32), dtype=np.uint8)  # {num_ex, num_sh} x 4
        else:
            t.entries[:, 224:256] = rng.integers(0, 256, (n, 32), dtype=np.uint8)  # owner keys
        t.entries[t.n_local:, 56:60] = rng.integers(0, 256, (t.pool_cap, 4), dtype=np.uint8)  # `head` of an overflow entry: never read
    return view


def hand_view(leaks=0, stride=256, lists=True):
    """buckets of 0, 1, 4, 5, 8, 9 and 68 rows; the inline entry at the head, in the middle, at the tail and unlinked; entries with
    one valid slot each; an all-invalid entry still linked; duplicate keys; `leaks` leaked entries; free and pend lists"""
    hash_size, pool_cap = 300, 200
    t = Tab(300, hash_size, pool_cap, stride)
    used_pool = 1 + 1 + 2 + 3 + 16 + 4 + 2 + 1 + 1 + 2 + (6 if lists else 0) + leaks
    assert used_pool <= pool_cap
    perm = np.random.default_rng(7).permutation(used_pool).tolist()
    take = lambda n: [perm.pop() for _ in range(n)]  # noqa: E731
    used = {}

    def put(b, seq, rows, valid=None):
        t.chain(b, seq)
        for i, (x, m) in enumerate(zip(seq, rows)):
            ks = keys_of(hash_size, (0, 1), b, m, used.get(b, 0))
            used[b] = used.get(b, 0) + m
            t.fill(b if x == "I" else t.pool(x), ks, None if valid is None else valid[i])

    put(0, take(1), [4], [[0, 0, 0, 0]])                       # 0 rows, head -> an entry without a valid slot
    put(1, ["I"], [1])
    put(2, ["I"], [4])                                          # already what the rule makes of it
    put(3, take(1) + ["I"], [1, 4])                             # 5 rows, the inline entry at the tail
    put(4, (lambda a: [a[0], "I", a[1]])(take(2)), [4, 2, 2])   # 8 rows, the inline entry in the middle
    put(5, take(3), [4, 4, 1])                                  # 9 rows, the inline entry unlinked
    put(6, ["I"] + take(16), [4] * 17)                          # 4 x 17 rows, right shape, scattered pool entries
    put(7, ["I"] + take(4), [4] * 5, [[0, 0, 1, 0], [0, 0, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]])  # one valid slot each
    put(8, ["I"] + take(2), [4, 4, 2], [[1, 1, 1, 1], [0, 0, 0, 0], [1, 1, 0, 0]])  # an all-invalid entry mid-chain
    p = take(1)
    put(9, p + ["I"], [2, 2])                                   # duplicate keys: the inline entry's first key := the head's first key
    t.entries[9, 0:8] = t.entries[t.pool(p[0]), 0:8]
    put(299, ["I"] + take(1), [4, 1])
    put(150, ["I"] + take(2), [4, 4, 4])                        # 12 rows in the first workgroup's last third
    if lists:
        t.lst(3, take(2), tag=4)
        t.lst(NLISTS + 7, take(3), tag=9)
        t.lst(2 * NLISTS + 1, take(1), tag=2)
    for p in take(leaks):  # leaked: below pool_top, in no chain and on no list; stale keys and links, no valid byte
        t.fill(t.pool(p), [900 + p], [0])
        t.set_u32(t.pool(p), 52, 5 + p)
    assert not perm
    t.top = used_pool
    wl = W.STORE if stride == 256 else W.SMALLBANK
    tabs = [t] if stride == 256 else [t, Tab(300, hash_size, pool_cap, stride)]
    return dress(View(wl, tabs), seed=leaks + 2)


def leak_only_view():
    return dress(one_change("store", "a")[0])


ACCEPTED = dict([(f"sound_{k}", lambda k=k: dress(sound_view(k))) for k in KINDS] + [(f"hand_{n}", lambda n=n: hand_view(n)) for n in LEAKS] +
                [("hand_smallbank", lambda: hand_view(1, stride=128)), ("hand_no_lists", lambda: hand_view(0, lists=False)),
                 ("leak_only", lambda: dress(one_change("store", "a")[0])), ("top_above_cap", lambda: dress(one_change("store", "m")[0]))])
REFUSED = [n for n in CHANGES if n not in "am"]  # every one-change copy of the verify tests that sets a gating count
DAMAGED = dict([(f"{k}_{n}", lambda k=k, n=n: dress(one_change(k, n)[0])) for k in KINDS for n in REFUSED] +
               [("bent", bent_view), ("truncated", truncated_view)])


def _same(got, want, where):
    assert got == want, (where, {k: (got[k], want[k]) for k in want if got[k] != want[k]})


# ------------------------------------------------------------------------------------------------ host form == numpy form
@pytest.mark.parametrize("name", list(ACCEPTED))
def test_host_form_equals_the_numpy_form_byte_for_byte(name):
    v = ACCEPTED[name]()
    ref, dry = v.copy(), v.copy()
    before = v.raw()
    inline_locks = [(t.entries[:t.n_local, 60:64].copy(), t.entries[:t.n_local, 96:128].copy() if t.stride == 128 else t.entries[:t.n_local, 224:256].copy())
                    for t in v.tabs]
    drc, dgot = host_compact(dry, DRY)
    assert dry.raw() == before  # a dry run changes nothing at all
    rc, got = host_compact(v)
    wrc, want = np_compact(ref)
    assert rc == drc == wrc == len(v.tabs), _lib.load().dint_last_error()
    for t, (g, d, w) in enumerate(zip(got, dgot, want)):
        _same(g, w, (name, t))
        _same(d, w, (name, "dry", t))
    assert v.raw() == ref.raw()  # the entries, pool_next, pool_top and the head words
    for t, (lockw, rest) in zip(v.tabs, inline_locks):  # lock bytes, counters and owner keys of the inline entries: as they were
        assert (t.entries[:t.n_local, 60:64] == lockw).all()
        assert (t.entries[:t.n_local, 96:128] if t.stride == 128 else t.entries[:t.n_local, 224:256]).tobytes() == rest.tobytes()
        ovf = t.entries[t.n_local:t.n_local + t.top]
        assert not ovf[:, 56:64].any() and not (ovf[:, 96:128] if t.stride == 128 else ovf[:, 224:256]).any()
    # afterwards: sound, nothing free, pending or leaked, the pool one range
    vrc, ver = host_verify(v)
    assert vrc == len(v.tabs)
    for g, r in zip(got, ver):
        assert is_clean(r) and r["free_entries"] == r["pending_entries"] == r["unaccounted"] == 0, r
        assert r["linked"] == r["pool_top"] == g["pool_top_after"] == g["overflow_after"] and r["rows"] == g["rows"]
    # idempotence: a second compaction changes nothing but the lists' tags
    once = v.copy()
    rc2, got2 = host_compact(v)
    assert rc2 == len(v.tabs)
    for a, b, g in zip(once.tabs, v.tabs, got2):
        assert a.entries.tobytes() == b.entries.tobytes() and a.pool_next.tobytes() == b.pool_next.tobytes() and a.top == b.top
        assert (b.heads() == a.heads() + (np.uint64(1) << np.uint64(32))).all()
        assert g["buckets_rewritten"] == 0 and g["holes_before"] == g["holes_after"] and g["pool_top_before"] == g["pool_top_after"]


def test_the_hand_built_buckets_are_what_the_docstring_says():
    v = hand_view(65)
    rc, (g,) = host_compact(v.copy(), DRY)
    assert rc == 1
    ks = sorted([0, 1, 4, 5, 8, 9, 68, 5, 6, 4, 5, 12])
    assert g["rows"] == sum(ks) and g["overflow_after"] == sum(max(0, (k + 3) // 4 - 1) for k in ks) == g["pool_top_after"]
    assert g["entries_after"] == sum((k + 3) // 4 for k in ks) and g["holes_after"] == sum(4 * ((k + 3) // 4) - k for k in ks)
    assert g["unaccounted_dropped"] == 65 and g["verify"]["free_entries"] == 2 and g["verify"]["pending_entries"] == 4
    assert g["pool_top_before"] == 39 + 65 and g["staging_bytes"] == 256 * g["overflow_after"]
    # every bucket but the two that are right already (1 row inline, 4 rows inline), the scattered 68 rows and the last ones
    assert g["buckets_rewritten"] == 7
    t = v.tabs[0]
    rc, _ = host_compact(v)
    assert rc == 1
    # duplicate keys: the head entry's row stays ahead of the inline entry's
    e = t.entries[9]
    assert e[0:8].tobytes() == e[16:24].tobytes() and t.u32(9, 48) == 0x01010101 and t.u32(9, 56) == 1 and t.u32(9, 52) == 0
    assert t.u32(0, 56) == 0 and t.u32(0, 48) == 0 and t.u32(5, 56) == 1  # the empty bucket; the unlinked inline entry is the head now
    assert t.u32(7, 48) == 0x01010101 and t.u32(7, 52) >= 2  # five single rows: a full inline entry and one overflow entry


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("name", list(DAMAGED))
def test_damaged_views_are_refused_and_not_a_byte_changes(name):
    v = DAMAGED[name]()
    before = v.raw()
    census = np_verify(v)
    assert any(c[k] for c in census for k in GATE)
    for flags in (0, DRY):
        rc, got = host_compact(v, flags)
        assert rc == ESTATE and b"nothing compacted" in _lib.load().dint_last_error()
        for g, c in zip(got, census):
            _same(g["verify"], c, name)  # the report is filled all the same ...
            assert all(g[k] == 0 for k in CFIELDS)  # ... and says that nothing moved
        assert v.raw() == before
    assert np_compact(v.copy())[0] == ESTATE


def test_one_changes_that_only_leak_are_accepted():
    for n in "am":
        v, want = one_change("store", n)
        assert not any(np_verify(v)[0][k] for k in GATE)
        rc, (g,) = host_compact(v)
        assert rc == 1 and g["unaccounted_dropped"] == want["unaccounted"] > 0 and g["pool_top_after"] == 68 - 1  # (bucket 12's six rows in two overflow entries: the inline entry and one)


def test_a_refusal_in_one_table_keeps_every_table_as_it_was():
    v = dress(sound_view("smallbank"))
    v.tabs[1].set_u32(1, 52, v.tabs[1].pool_cap + 7)  # table 1 has a bad chain; table 0 is sound and full of holes
    before = v.raw()
    rc, got = host_compact(v)
    assert rc == ESTATE and got[1]["verify"]["bad_chains"] == 1 and got[0]["rows"] == 0 and v.raw() == before


def test_views_that_fail_the_check_and_bad_arguments():
    L = _lib.load()
    out = (_lib.TableCompact * 5)()

    def rc_of(change, flags=0, cap=5):
        v = sound_view()
        cv = v.c_view()
        change(cv)
        before = v.raw()
        rc = L.dint_state_compact_view_host(C.byref(cv), out, cap, flags)
        assert rc >= 0 or v.raw() == before
        return rc

    def st(field, value, table=True):
        def f(cv):
            setattr(cv.table[0] if table else cv, field, value)
        return f

    assert rc_of(lambda cv: None) == 1
    for ch in (st("stride", 128), st("val_size", 8), st("n_local", 299), st("hash_size", 0), st("entries", None), st("ctl", None),
               st("pool_next", None), st("workload", int(W.TATP), False), st("workload", int(W.FASST), False), st("n_tables", 2, False),
               st("shard_count", 0, False), st("shard_index", 1, False), st("shard_count", 3, False)):
        assert rc_of(ch) == EINVAL
    v = sound_view()
    for field, by in (("entries", 8), ("ctl", 4), ("pool_next", 2)):
        cv = v.c_view()
        setattr(cv.table[0], field, getattr(cv.table[0], field) + by)
        assert L.dint_state_compact_view_host(C.byref(cv), out, 5, 0) == EINVAL and b"aligned" in L.dint_last_error()
    assert rc_of(lambda cv: None, cap=0) == EINVAL and b"room for" in L.dint_last_error()
    assert rc_of(lambda cv: None, flags=2) == EINVAL  # an unknown flag
    assert L.dint_state_compact_view_host(None, out, 5, 0) == EINVAL
    assert L.dint_state_compact_view_host(C.byref(v.c_view()), None, 5, 0) == EINVAL


def test_struct_layout_and_flag_name():
    assert C.sizeof(_lib.TableCompact) == 512 and _lib.TableCompact.rows.offset == 256 and _lib.TableCompact.staging_bytes.offset == 256 + 11 * 8
    assert _lib.TableCompact.reserved.offset == 256 + 12 * 8
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    abi = open(os.path.join(root, "include", "dint_abi.h")).read()
    assert "#define DINT_COMPACT_DRY_RUN 1u" in abi and "#define DINT_ABI_VERSION 5 " in abi and _lib.COMPACT_DRY_RUN == 1


# ------------------------------------------------------------------------------------------------ recovery: the sums and the advice
class _FakeEngine:
    workload = W.TATP

    def __init__(self, compact, stats=None, hash_sizes=None):
        self._c, self._s, self._h = compact, stats, hash_sizes

    def state_compact(self, dry_run=False):
        self.dry = dry_run
        return [dict(r, verify=dict(r["verify"])) for r in self._c]

    def state_stats(self):
        return [dict(s) for s in self._s]

    def hash_size(self, t):
        return self._h[t]


def test_compact_tables_adds_the_reports_of_a_set():
    a = np_compact(hand_view(1), dry=True)[1]
    b = np_compact(hand_view(65), dry=True)[1]
    ea, eb = _FakeEngine(a), _FakeEngine(b)
    s = recovery.compact_tables([ea, eb], dry_run=True)
    assert ea.dry and eb.dry and s["engines"] == [a, b]
    (t,) = s["tables"]
    for k in CFIELDS:
        assert t[k] == a[0][k] + b[0][k]
    assert t["verify"]["unaccounted"] == 66 and t["verify"]["longest_list"] == max(a[0]["verify"]["longest_list"], b[0]["verify"]["longest_list"])
    assert recovery.compact_tables([]) == {"tables": [], "engines": []}


def _stats(rows, entries, overflow, pool_cap, pool_top, locks=0):
    return dict(buckets=100, buckets_empty=0, rows=rows, entries=entries, overflow_entries=overflow, holes=4 * entries - rows, inline_first=0,
                inline_unlinked=0, hit_entries=rows, shadowed_rows=0, buckets_unchecked=0, longest_chain=3, longest_chain_bucket=0, most_rows=9,
                locks_held=locks, pool_cap=pool_cap, pool_top=pool_top, chain_hist=[0] * 17, rows_hist=[0] * 33)


def _compact(rows, e0, e1, o0, o1, top0):
    c = {k: 0 for k in CFIELDS}
    c.update(rows=rows, entries_before=e0, entries_after=e1, overflow_before=o0, overflow_after=o1, pool_top_before=top0, pool_top_after=o1,
             holes_before=4 * e0 - rows, holes_after=4 * e1 - rows)
    c["verify"] = {"unaccounted": 0, "longest_list": 0}
    return c


def test_compact_advice_is_policy_over_one_stats_and_one_dry_run():
    hs = [100]
    # the load is fine (2 rows per bucket), but half of every entry is a hole and the pool's top is at its end
    churned = _FakeEngine([_compact(200, 150, 100, 60, 0, 400)], [_stats(200, 150, 60, 400, 400)], hs)
    a = recovery.compact_advice([churned])
    assert a["action"] == "compact" and churned.dry and a["load"] == [2.0] and a["hole_share"] == pytest.approx(200 / 600) and a["pool_top_fill"] == 1.0
    assert a["pool_top_fill_after"] == 0.0 and a["n_rows"] == recovery.advise_n_rows(W.TATP, [200])
    # the same table with nothing to gain
    tidy = _FakeEngine([_compact(200, 100, 100, 0, 0, 0)], [_stats(200, 100, 0, 400, 0)], hs)
    assert recovery.compact_advice([tidy])["action"] == "none"
    # too few buckets: compaction cannot help
    full = _FakeEngine([_compact(900, 300, 225, 200, 125, 400)], [_stats(900, 300, 200, 400, 400)], hs)
    a = recovery.compact_advice([full])
    r = recovery.rehash_advice([full])
    assert a["action"] == "rehash" and r["needed"] and a["n_rows"] == r["n_rows"]
    # the thresholds are arguments
    assert recovery.compact_advice([churned], max_hole_share=0.9, max_pool_top_fill=1.0)["action"] == "none"
    assert recovery.compact_advice([tidy], max_rows_per_bucket=1.5)["action"] == "rehash"
    # a pool that stays too full after a compaction: the chains need more buckets
    stuck = _FakeEngine([_compact(390, 330, 330, 230, 230, 400)], [_stats(390, 330, 230, 400, 400)], hs)
    assert recovery.compact_advice([stuck])["action"] == "rehash"


# ------------------------------------------------------------------------------------------------ churn on the host build
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "kv_compact_host.cc")
LIB = os.path.join(HERE, "native", "libkv_compact_host.so")


@pytest.fixture(scope="module")
def kvh():
    deps = [SRC, os.path.join(HERE, "native", "kv_view_host.cc"), os.path.join(HERE, "native", "kv_core_host.cc"),
            os.path.join(HERE, "..", "dint_amd", "csrc", "dint_kv_core.h")]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", LIB, SRC])
    L = C.CDLL(LIB)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.kvh_create.restype, L.kvh_create.argtypes = vp, [u64, u32, u32]
    L.kvh_destroy.argtypes = [vp]
    L.kvh_insert.argtypes = [vp, u64, u64, vp, u32]
    L.kvh_delete.argtypes = [vp, u64, u64]
    L.kvh_get.argtypes = [vp, u64, u64, vp, vp]
    L.kvh_set.argtypes = [vp, u64, u64, vp]
    L.kvh_rotate.argtypes = [vp]
    L.kvh_pool_top.restype, L.kvh_pool_top.argtypes = u32, [vp]
    L.kvh_dump.restype, L.kvh_dump.argtypes = u64, [vp, vp, vp, vp, u64]
    L.kvh_view_fill.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(vp)]
    L.kvh_ctl_store.argtypes = [vp, vp]
    L.kvh_set_lock_bytes.argtypes = [vp, u64, u32]
    L.kvh_get_lock_bytes.restype, L.kvh_get_lock_bytes.argtypes = u32, [vp, u64]
    return L


def _kvh_view(L, h, nb, cap):
    ctl = np.zeros(_lib.VIEW_CTL_BYTES, np.uint8)
    ent, nxt = C.c_void_p(), C.c_void_p()
    L.kvh_view_fill(h, ctl.ctypes.data, C.byref(ent), C.byref(nxt))
    v = _lib.TablesView()
    v.workload, v.n_tables, v.shard_index, v.shard_count = int(W.STORE), 1, 0, 1
    tv = v.table[0]
    tv.entries, tv.pool_next, tv.ctl = ent.value, nxt.value, ctl.ctypes.data
    tv.n_local, tv.hash_size, tv.pool_cap, tv.stride, tv.val_size = nb, nb, cap, 256, 40
    return v, ctl


def _dump(L, h, sort=False):
    n = L.kvh_dump(h, None, None, None, 0)
    keys = np.zeros(n, "<u8"); vers = np.zeros(n, "<u4"); vals = np.zeros((n, 40), "u1")
    assert L.kvh_dump(h, keys.ctypes.data, vers.ctypes.data, vals.ctypes.data, n) == n
    if sort:
        return sorted(zip(keys.tolist(), vers.tolist(), [v.tobytes() for v in vals]))
    return keys.tobytes(), vers.tobytes(), vals.tobytes()


def test_churn_on_the_host_build_compacted_and_driven_on_beside_a_twin(kvh):
    L, nb, cap = kvh, 13, 600
    a, b = L.kvh_create(nb, cap, 40), L.kvh_create(nb, cap, 40)
    rng = np.random.default_rng(11)
    pool = (np.arange(1, 401, dtype=np.uint64) * np.uint64(7919)).tolist()
    bucket = dict(zip(pool, np_bucket(pool, nb).astype(np.int64).tolist()))
    live, val = set(), np.zeros(40, np.uint8)
    for bk in range(nb):
        L.kvh_set_lock_bytes(a, bk, 0x01000100 + bk)
        L.kvh_set_lock_bytes(b, bk, 0x01000100 + bk)
    for step in range(6000):
        k = pool[int(rng.integers(len(pool)))]
        val[:] = (step * 7 + np.arange(40)) & 0xFF
        for h in (a, b):
            if k in live:
                assert L.kvh_delete(h, bucket[k], k) == 0
            else:
                assert L.kvh_insert(h, bucket[k], k, val.ctypes.data, step) == 0
        live ^= {k}
        if step % 97 == 0:
            L.kvh_rotate(a); L.kvh_rotate(b)
    order = _dump(L, a)
    assert order == _dump(L, b)
    v, ctl = _kvh_view(L, a, nb, cap)
    out = (_lib.TableCompact * 5)()
    assert _lib.load().dint_state_compact_view_host(C.byref(v), out, 5, 0) == 1, _lib.load().dint_last_error()
    L.kvh_ctl_store(a, ctl.ctypes.data)
    g = out[0].as_dict()
    print(g)
    assert g["rows"] == len(live) and g["holes_before"] > g["holes_after"] and g["pool_top_before"] > g["pool_top_after"] == L.kvh_pool_top(a)
    assert g["verify"]["free_entries"] + g["verify"]["pending_entries"] > 0 and g["buckets_rewritten"] > 0
    assert _dump(L, a) == order  # chain order kept: the same rows in the same sequence
    assert [L.kvh_get_lock_bytes(a, bk) for bk in range(nb)] == [0x01000100 + bk for bk in range(nb)]
    ver = (_lib.TableVerify * 5)()
    v, _ = _kvh_view(L, a, nb, cap)
    assert _lib.load().dint_state_verify_view_host(C.byref(v), ver, 5, 0) == 1
    r = ver[0].as_dict()
    assert is_clean(r) and r["linked"] == r["pool_top"] == g["pool_top_after"] and r["free_entries"] == r["pending_entries"] == 0 and r["rows"] == len(live)
    # on beside the uncompacted twin: reads, sets, inserts and deletes of fresh keys (none holds a duplicate row)
    fresh = (np.arange(1, 3001, dtype=np.uint64) * np.uint64(104729) + np.uint64(5)).tolist()
    fb = dict(zip(fresh, np_bucket(fresh, nb).astype(np.int64).tolist()))
    bucket.update(fb)
    known, got_a, got_b = sorted(live), np.zeros(40, np.uint8), np.zeros(40, np.uint8)
    ver_a, ver_b = C.c_uint32(), C.c_uint32()
    fresh_live = []
    for step in range(6000):
        op = int(rng.integers(4))
        if op == 0 or (op == 3 and not fresh_live):  # read: a stored key or a missing one
            k = known[int(rng.integers(len(known)))] if rng.integers(4) else fresh[int(rng.integers(len(fresh)))]
            ra = L.kvh_get(a, bucket[k], k, got_a.ctypes.data, C.byref(ver_a))
            rb = L.kvh_get(b, bucket[k], k, got_b.ctypes.data, C.byref(ver_b))
            assert ra == rb and (ra or (ver_a.value == ver_b.value and got_a.tobytes() == got_b.tobytes()))
        elif op == 1:
            k = known[int(rng.integers(len(known)))]
            val[:] = (step * 11 + np.arange(40)) & 0xFF
            assert L.kvh_set(a, bucket[k], k, val.ctypes.data) == L.kvh_set(b, bucket[k], k, val.ctypes.data) == 0
        elif op == 2:
            k = fresh[step % len(fresh)]
            if k in fresh_live:
                continue
            val[:] = (step * 13 + np.arange(40)) & 0xFF
            assert L.kvh_insert(a, bucket[k], k, val.ctypes.data, step) == L.kvh_insert(b, bucket[k], k, val.ctypes.data, step) == 0
            fresh_live.append(k)
        else:
            k = fresh_live.pop(int(rng.integers(len(fresh_live))))
            assert L.kvh_delete(a, bucket[k], k) == L.kvh_delete(b, bucket[k], k) == 0
        if step % 97 == 0:
            L.kvh_rotate(a); L.kvh_rotate(b)
    assert _dump(L, a, sort=True) == _dump(L, b, sort=True)  # the same row multiset
    v, _ = _kvh_view(L, a, nb, cap)
    assert _lib.load().dint_state_verify_view_host(C.byref(v), ver, 5, 0) == 1 and is_clean(ver[0].as_dict())
    L.kvh_destroy(a); L.kvh_destroy(b)


# ------------------------------------------------------------------------------------------------ the fixtures as a file
def all_cases():
    """(name, view, flags): everything above that the device and the stand-alone program are shown as well"""
    c = [(n, f(), 0) for n, f in ACCEPTED.items()]
    c += [(f"dry_{n}", f(), DRY) for n, f in list(ACCEPTED.items())[:4]]
    c += [(f"refused_{n}", f(), 0) for n, f in DAMAGED.items()]
    return c


def expected(view, flags):
    """(rc, reports, the view afterwards) by the numpy form"""
    after = view.copy()
    rc, rep = np_compact(after, dry=bool(flags & DRY))
    return rc, rep, after


def report_words(r):
    from test_state_verify_host import FIELDS

    return [r["verify"][k] for k in FIELDS] + [0] * 14 + [r[k] for k in CFIELDS] + [0] * 20


if __name__ == "__main__":
    # u64 cases; per case: i32 {workload, n_tables, shard_index, shard_count, flags, rc}; per table u64 {n_local, hash_size, pool_cap,
    # stride, val_size}, entries, pool_next, ctl; then per table the numpy report as 64 u64; then per table entries, pool_next, ctl
    # as they must be afterwards
    cases = all_cases()
    with open(sys.argv[1], "wb") as f:
        f.write(struct.pack("<Q", len(cases)))
        for _, v, flags in cases:
            rc, rep, after = expected(v, flags)
            f.write(struct.pack("<6i", int(v.workload), len(v.tabs), v.shard[0], v.shard[1], flags, rc))
            for t in v.tabs:
                f.write(struct.pack("<5Q", t.n_local, t.hash_size, t.pool_cap, t.stride, SHAPE[v.workload][2]))
                f.write(t.entries.tobytes() + t.pool_next.tobytes() + t.ctl.tobytes())
            for r in rep:
                f.write(struct.pack("<64Q", *report_words(r)))
            for t in after.tabs:
                f.write(t.entries.tobytes() + t.pool_next.tobytes() + t.ctl.tobytes())
    print(len(cases), "views")
