"""The table verify's rule without a GPU (dint_amd/csrc/state_verify.h through dint_state_verify_view_host, include/dint_driver.h)
against a numpy / Python form of the census and of the reclaim over a view's raw bytes, written from the layout comment of
dint_kv_core.h and the rule's description alone: it shares no code with the rule and takes its hash from tests/shard_double.py
(np_bucket of test_state_image_host.py).  Hand-built tables -- a sound one and one-change copies of it, each with the counter
it is about asserted by hand as well --, reclaim around the list count, and the host build of dint_kv_core.h driven through
random churn (tests/native/kv_view_host.cc).  Every comparison is exact.

`python tests/test_state_verify_host.py FILE` writes every view below, bent and truncated copies included, with the numpy form's
reports (and, for a reclaim, the bytes afterwards) into FILE, for the stand-alone sanitizer program tests/native/state_verify_main.cc."""
import copy
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

W = wire.Workload
EINVAL, ESTATE = -1, -5
RECLAIM = 1
NLISTS, MAX_CHAIN = 64, 4096
SHAPE = {W.STORE: (1, 256, 40), W.TATP: (5, 256, 40), W.SMALLBANK: (2, 128, 8)}  # tables, stride, value size
FIELDS = ("pool_cap", "pool_top", "rows", "linked", "free_entries", "pending_entries", "unaccounted", "longest_list", "bad_chains",
          "cross_linked", "linked_beyond_top", "list_bad_links", "stray_valid_entries", "stray_rows", "misplaced_rows", "odd_valid_bytes",
          "reclaimed", "stray_rows_cleared")
VIOLATIONS = recovery.VERIFY_VIOLATIONS
REFUSING = ("bad_chains", "cross_linked", "linked_beyond_top", "list_bad_links")


# ------------------------------------------------------------------------------------------------ a view as numpy arrays
class Tab:
    """one table: entries [n_local + pool_cap, stride] u8, pool_next [pool_cap] u4, ctl [1600] u8 (pool_top at 0, the 192 head
    words {tag:32, link:32} at 64: 64 free lists, pend set 0, pend set 1)"""

    def __init__(self, n_local, hash_size, pool_cap, stride):
        self.n_local, self.hash_size, self.pool_cap, self.stride = n_local, hash_size, pool_cap, stride
        self.entries = np.zeros((n_local + pool_cap, stride), np.uint8)
        self.pool_next = np.zeros(pool_cap, "<u4")
        self.ctl = np.zeros(_lib.VIEW_CTL_BYTES, np.uint8)

    # header words of entry row e (inline entry of bucket b: row b; pool entry p: row n_local + p)
    def u32(self, e, off):
        return int(self.entries[e, off:off + 4].view("<u4")[0])

    def set_u32(self, e, off, v):
        self.entries[e, off:off + 4] = np.frombuffer(struct.pack("<I", v & 0xFFFFFFFF), np.uint8)

    def pool(self, p):
        return self.n_local + p

    @property
    def top(self):
        return int(self.ctl[:4].view("<u4")[0])

    @top.setter
    def top(self, v):
        self.ctl[:4] = np.frombuffer(struct.pack("<I", v), np.uint8)

    def heads(self):
        return self.ctl[64:64 + 8 * 3 * NLISTS].view("<u8")

    def fill(self, e, keys, valid=None):
        """keys into slots 0.. of entry row e, their valid bytes 1 (or `valid`), versions and a value byte to tell slots apart"""
        for i, k in enumerate(keys):
            self.entries[e, 8 * i:8 * i + 8] = np.frombuffer(struct.pack("<Q", int(k)), np.uint8)
            self.set_u32(e, 32 + 4 * i, i + 1)
            self.entries[e, 48 + i] = 1 if valid is None else valid[i]
            self.entries[e, 64 + i * ((self.stride - 64) // 8)] = 0xA0 + i

    def chain(self, b, seq):
        """bucket b's chain: seq of "I" (the inline entry) or pool indices, in chain order"""
        links = [1 if x == "I" else x + 2 for x in seq] + [0]
        self.set_u32(b, 56, links[0])
        for x, nxt in zip(seq, links[1:]):
            self.set_u32(b if x == "I" else self.pool(x), 52, nxt)

    def lst(self, li, seq, tag=5):
        """list li (0..63 free, 64..127 pend set 0, 128..191 pend set 1) = the pool entries of seq, head first"""
        self.heads()[li] = (tag << 32) | (seq[0] + 2 if seq else 0)
        for p, nxt in zip(seq, list(seq[1:]) + [None]):
            self.pool_next[p] = 0 if nxt is None else nxt + 2


class View:
    def __init__(self, workload, tabs, shard=(0, 1)):
        self.workload, self.tabs, self.shard = workload, tabs, shard
        self.meta = {}

    def copy(self):
        return copy.deepcopy(self)

    def raw(self):
        return [(t.entries.tobytes(), t.pool_next.tobytes(), t.ctl.tobytes()) for t in self.tabs]

    def c_view(self, ptr=lambda a: a.ctypes.data):
        v = _lib.TablesView()
        v.workload, v.n_tables, (v.shard_index, v.shard_count) = int(self.workload), len(self.tabs), self.shard
        _, _, val_size = SHAPE[self.workload]
        for i, t in enumerate(self.tabs):
            tv = v.table[i]
            tv.entries, tv.pool_next, tv.ctl = ptr(t.entries), ptr(t.pool_next), ptr(t.ctl)
            tv.n_local, tv.hash_size, tv.pool_cap, tv.stride, tv.val_size = t.n_local, t.hash_size, t.pool_cap, t.stride, val_size
        return v


def host_verify(view, flags=0, cap=5):
    out = (_lib.TableVerify * 5)()
    L = _lib.load()
    rc = L.dint_state_verify_view_host(C.byref(view.c_view()), out, cap, flags)
    return rc, [out[t].as_dict() for t in range(len(view.tabs))]


# ------------------------------------------------------------------------------------------------ the numpy / Python form
def _valid_slots(e):
    return e[48:52] != 0


def np_verify_table(t, shard):
    """the census of one table from its bytes: (report, owner) -- owner[p] = 0 unclaimed, > 0 a chain's, < 0 a list's"""
    idx, cnt = shard
    r = {k: 0 for k in FIELDS}
    raw_top = t.top
    top = min(raw_top, t.pool_cap)
    r["pool_cap"], r["pool_top"] = t.pool_cap, raw_top
    owner = [0] * t.pool_cap
    ent = t.entries
    for b in range(t.n_local):
        link, steps, seen_inline, bad = t.u32(b, 56), 0, False, False
        while link:
            if steps >= MAX_CHAIN:
                bad = True
                break
            steps += 1
            if link == 1:
                if seen_inline:
                    bad = True
                    break
                seen_inline, e = True, ent[b]
            else:
                p = link - 2
                if p >= t.pool_cap:
                    bad = True
                    break
                e = ent[t.n_local + p]
                if owner[p] == 0:
                    owner[p] = b + 1
                    r["linked"] += 1
                    r["linked_beyond_top"] += p >= top
                elif owner[p] == b + 1:  # the chain has come back to one of its own entries: nothing is counted twice
                    link = int(e[52:56].view("<u4")[0])
                    continue
                else:
                    r["cross_linked"] += 1
            v = _valid_slots(e)
            if v.any():
                g = np_bucket(e[:32].view("<u8")[v], t.hash_size).astype(np.int64)
                home = np.where(g % cnt == idx, g // cnt, -1)
                r["rows"] += int(v.sum())
                r["misplaced_rows"] += int((home != b).sum())
                r["odd_valid_bytes"] += int((e[48:52] > 1).sum())
            link = int(e[52:56].view("<u4")[0])
        if bad:
            r["bad_chains"] += 1
        elif not seen_inline and _valid_slots(ent[b]).any():
            r["stray_valid_entries"] += 1
            r["stray_rows"] += int(_valid_slots(ent[b]).sum())
    heads = t.heads()
    for li in range(3 * NLISTS):
        link, n = int(heads[li]) & 0xFFFFFFFF, 0
        while link:
            if link == 1 or link - 2 >= t.pool_cap:
                r["list_bad_links"] += 1
                break
            p = link - 2
            if owner[p] != 0:
                r["cross_linked"] += 1
                break
            owner[p] = -(li + 1)
            n += 1
            r["linked_beyond_top"] += p >= top
            link = int(t.pool_next[p])
        r["free_entries" if li < NLISTS else "pending_entries"] += n
        r["longest_list"] = max(r["longest_list"], n)
    for p in range(t.pool_cap):
        v = int(_valid_slots(ent[t.n_local + p]).sum())
        if owner[p] == 0 and p < top:
            r["unaccounted"] += 1
        if owner[p] <= 0 and v:
            r["stray_valid_entries"] += 1
            r["stray_rows"] += v
    return r, owner


def np_verify(view):
    return [np_verify_table(t, view.shard)[0] for t in view.tabs]


def np_reclaim(view):
    """the reports of a reclaim call and, when it is not refused, the view's bytes rewritten as the rule says; returns (rc, reports)"""
    pairs = [np_verify_table(t, view.shard) for t in view.tabs]
    if any(r[k] for r, _ in pairs for k in REFUSING):
        return ESTATE, [r for r, _ in pairs]
    for t, (r, owner) in zip(view.tabs, pairs):
        top = min(t.top, t.pool_cap)
        U = [p for p in range(top) if owner[p] == 0]
        n = len(U)
        old = t.heads()[:NLISTS].copy()
        for rank, p in enumerate(U):
            r["stray_rows_cleared"] += int(_valid_slots(t.entries[t.n_local + p]).sum())
            t.pool_next[p] = U[rank + NLISTS] + 2 if rank + NLISTS < n else int(old[rank % NLISTS]) & 0xFFFFFFFF
            t.entries[t.n_local + p, 48:56] = 0
        for li in range(min(n, NLISTS)):
            t.heads()[li] = (((int(old[li]) >> 32) + 1) << 32) | (U[li] + 2)
        r["reclaimed"] = n
    return len(view.tabs), [r for r, _ in pairs]


def assert_identities(r):
    """what every report satisfies, whatever made it"""
    if r["cross_linked"] == 0 and r["bad_chains"] == 0 and r["list_bad_links"] == 0:
        assert r["linked"] + r["free_entries"] + r["pending_entries"] - r["linked_beyond_top"] + r["unaccounted"] == min(r["pool_top"], r["pool_cap"]), r
    assert r["stray_rows"] >= r["stray_valid_entries"]


def is_clean(r):
    return all(r[k] == 0 for k in VIOLATIONS) and r["unaccounted"] == 0


# ------------------------------------------------------------------------------------------------ hand-built tables
_KEYS = {}


def keys_of(hash_size, shard, b, n, skip=0):
    """n keys whose home is local bucket b (searched: hash % hash_size == b * count + index)"""
    if (hash_size, shard) not in _KEYS:
        cand = np.arange(1, 400_000, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345)
        g = np_bucket(cand, hash_size).astype(np.int64)
        mine = g % shard[1] == shard[0]
        _KEYS[(hash_size, shard)] = (cand[mine], g[mine] // shard[1])
    cand, loc = _KEYS[(hash_size, shard)]
    out = cand[loc == b][skip:skip + n]
    assert len(out) == n
    return out.tolist()


def sound_table(stride=256, shard=(0, 1), hash_size=300, pool_cap=200, pool_top=150, seed=3, filler_list=33):
    """the sound table: (Tab, meta).  68 overflow entries in chains, 82 on lists, whatever else lies below pool_top on free list
    `filler_list`; the pool entries are dealt out in a shuffled order"""
    n_local = -(-hash_size // shard[1])
    t = Tab(n_local, hash_size, pool_cap, stride)
    t.top = pool_top
    perm = np.random.default_rng(seed).permutation(pool_top).tolist()
    take = lambda n: [perm.pop() for _ in range(n)]  # noqa: E731
    meta = {"chains": {}, "lists": {}}
    used = {}

    def put(b, seq, rows):
        """bucket b's chain seq with rows[i] valid slots in entry i"""
        t.chain(b, seq)
        for x, m in zip(seq, rows):
            ks = keys_of(hash_size, shard, b, m, used.get(b, 0))
            used[b] = used.get(b, 0) + m
            t.fill(b if x == "I" else t.pool(x), ks)
        meta["chains"][b] = list(seq)

    for b in list(range(0, 10)) + [n_local - 1]:  # the inline entry only
        put(b, ["I"], [1 + b % 4])
    put(10, ["I"] + take(2), [4, 4, 2])      # inline first, two overflow entries
    put(11, (lambda a: [a[0], "I", a[1]])(take(2)), [3, 4, 4])  # an overflow head, the inline entry mid-chain
    put(12, take(2), [2, 4])                 # the inline entry unlinked (and empty)
    for b in list(range(20, 50)) + [n_local - 40]:  # 31 more chains, one of them in the second workgroup
        put(b, ["I"] + take(2), [4, 4, 1 + b % 4])
    for li, n in ((0, 3), (63, 1), (9, 6), (NLISTS + 5, 2), (2 * NLISTS + 7, 70)):
        meta["lists"][li] = take(n)
        t.lst(li, meta["lists"][li], tag=li + 1)
    if perm:
        meta["lists"][filler_list] = take(len(perm))
        t.lst(filler_list, meta["lists"][filler_list], tag=9)
    assert not perm
    return t, meta


def sound_view(kind="store"):
    if kind == "store":
        t, m = sound_table()
        v = View(W.STORE, [t])
    elif kind == "sharded":
        t, m = sound_table(shard=(1, 3), hash_size=899)
        v = View(W.STORE, [t], shard=(1, 3))
    else:  # the smallbank shape: two tables of 128-byte entries
        t, m = sound_table(stride=128)
        t2, _ = sound_table(stride=128, seed=4)
        v = View(W.SMALLBANK, [t, t2])
    v.meta = m
    return v


def one_change(kind, name):
    """(view, {counter: value asserted by hand}) -- a copy of the sound view with ONE thing changed"""
    v = sound_view(kind)
    t, m = v.tabs[0], v.meta
    ch, ls = m["chains"], m["lists"]
    cap, n_local = t.pool_cap, t.n_local
    if name in ("a", "b"):  # five entries unlinked from free list 9
        cut = ls[9][1:]
        t.pool_next[ls[9][0]] = 0
        want = {"unaccounted": 5}
        if name == "b":  # ... one of them with two stale valid bytes
            t.entries[t.pool(cut[2]), 48] = 1
            t.entries[t.pool(cut[2]), 50] = 1
            want.update(stray_valid_entries=1, stray_rows=2)
    elif name == "c":  # bucket 10's tail points at the last overflow entry of bucket 20
        y = ch[20][-1]
        t.set_u32(t.pool(ch[10][-1]), 52, y + 2)
        want = {"cross_linked": 1, "misplaced_rows": int(_valid_slots(t.entries[t.pool(y)]).sum())}
    elif name == "d":  # a chain's tail points at the middle entry of free list 0: the entry behind it is lost to the list
        t.set_u32(t.pool(ch[10][-1]), 52, ls[0][1] + 2)
        want = {"cross_linked": 1, "unaccounted": 1}
    elif name == "e":  # free list 63's only entry leads on to free list 0's tail
        t.pool_next[ls[63][0]] = ls[0][2] + 2
        want = {"cross_linked": 1}
    elif name == "f":  # a pend list's last pool_next points at its first entry
        t.pool_next[ls[NLISTS + 5][-1]] = ls[NLISTS + 5][0] + 2
        want = {"cross_linked": 1}
    elif name == "g":  # a chain link to p = 170, between pool_top and pool_cap
        t.set_u32(0, 52, 170 + 2)
        want = {"linked_beyond_top": 1}
    elif name == "h":  # a chain link to p = pool_cap + 5 and one to 0xFFFFFFFF
        t.set_u32(1, 52, cap + 5 + 2)
        t.set_u32(2, 52, 0xFFFFFFFF)
        want = {"bad_chains": 2}
    elif name == "i":  # a free head of 1 and a pool_next of pool_cap + 9
        t.heads()[20] = (7 << 32) | 1
        t.pool_next[ls[9][-1]] = cap + 9
        want = {"list_bad_links": 2}
    elif name == "j":  # a two-entry chain cycle
        t.set_u32(t.pool(ch[21][2]), 52, ch[21][1] + 2)
        want = {"bad_chains": 1}
    elif name == "k":  # one key swapped for a key of another bucket (sharded: of another shard)
        if kind == "sharded":
            other = np.arange(1, 200, dtype=np.uint64)
            other = int(other[np_bucket(other, t.hash_size).astype(np.int64) % 3 != 1][0])
        else:
            other = keys_of(t.hash_size, v.shard, 77, 1)[0]
        t.entries[t.pool(ch[30][1]), 8:16] = np.frombuffer(struct.pack("<Q", other), np.uint8)
        want = {"misplaced_rows": 1}
    elif name == "l":  # a valid byte of 2
        t.entries[t.pool(ch[30][1]), 49] = 2
        want = {"odd_valid_bytes": 1, "rows": np_verify(sound_view(kind))[0]["rows"]}
    elif name == "m":  # pool_top above pool_cap: reported raw, used clamped
        t.top = cap + 3
        want = {"pool_top": cap + 3, "unaccounted": cap - 150}
    elif name == "n":  # an unlinked inline entry with a valid byte
        t.entries[12, 48] = 1
        want = {"stray_valid_entries": 1, "stray_rows": 1}
    else:
        raise KeyError(name)
    return v, want


CHANGES = "abcdefghijklmn"
KINDS = ("store", "sharded", "smallbank")
LEAKS = (0, 1, 63, 64, 65, 300)


def leaked_view(n):
    """pool_cap 700, 650 handed out, 500 of them on free list 33: the last n of that list cut off, some with stale header bytes"""
    t, m = sound_table(pool_cap=700, pool_top=650)
    fl = m["lists"][33]
    if n:
        keep, cut = fl[:len(fl) - n], fl[len(fl) - n:]
        t.pool_next[keep[-1]] = 0
        for i, p in enumerate(cut):
            if i % 3 == 0:  # stale: keys, a valid byte or two, a link -- the 8 bytes {validw, next} go, the rest stays
                t.fill(t.pool(p), [900 + i, 901 + i][:1 + i % 2])
                t.set_u32(t.pool(p), 52, 7 + i)
    v = View(W.STORE, [t])
    v.meta = m
    return v


def bent_view():
    """every link of the sound view far outside: the header words at 52..59 of every entry, every pool_next, every head word"""
    v = sound_view()
    t = v.tabs[0]
    t.entries[:, 52:60] = 0xEE
    t.pool_next[:] = 0xEEEEEEEE
    t.heads()[:] = 0xEEEEEEEEEEEEEEEE
    return v


def truncated_view():
    """the sound view cut to half its pool: the links that now leave the pool must be refused before anything is read"""
    v = sound_view()
    t = v.tabs[0]
    h = Tab(t.n_local, t.hash_size, t.pool_cap // 2, t.stride)
    h.entries[:] = t.entries[:t.n_local + h.pool_cap]
    h.pool_next[:] = t.pool_next[:h.pool_cap]
    h.ctl[:] = t.ctl
    v.tabs[0] = h
    return v


def _same(got, want, where):
    assert got == want, (where, {k: (got[k], want[k]) for k in want if got[k] != want[k]})


# ------------------------------------------------------------------------------------------------ the census
@pytest.mark.parametrize("kind", KINDS)
def test_sound_table_is_clean(kind):
    v = sound_view(kind)
    before = v.raw()
    rc, got = host_verify(v)
    want = np_verify(v)
    assert rc == len(v.tabs)
    for t, (g, w) in enumerate(zip(got, want)):
        _same(g, w, (kind, t))
        assert_identities(g)
        assert is_clean(g), g
        assert g["pool_cap"] == 200 and g["pool_top"] == 150 and g["linked"] == 68 and g["free_entries"] == 10 and g["pending_entries"] == 72
        assert g["longest_list"] == 70 and g["rows"] > 200 and g["reclaimed"] == 0
    assert v.raw() == before  # read-only
    # the shapes the sound table is said to hold
    t, m = v.tabs[0], v.meta
    assert t.u32(10, 56) == 1 and t.u32(11, 56) >= 2 and "I" in m["chains"][11][1:] and "I" not in m["chains"][12] and t.u32(12, 48) == 0
    assert t.n_local == 300 and any(b >= 256 for b in m["chains"])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", CHANGES)
def test_one_change_copies(kind, name):
    v, hand = one_change(kind, name)
    before = v.raw()
    rc, got = host_verify(v)  # ((f): the call returns)
    want = np_verify(v)
    assert rc == len(v.tabs)
    for t, (g, w) in enumerate(zip(got, want)):
        _same(g, w, (kind, name, t))
        assert_identities(g)
    for k, x in hand.items():
        assert got[0][k] == x, (name, k, got[0])
    for k in VIOLATIONS:  # ONE change: no other violation appears
        if k not in hand:
            assert got[0][k] == 0, (name, k, got[0])
    if len(v.tabs) > 1:
        assert is_clean(got[1])
    assert v.raw() == before


@pytest.mark.parametrize("maker", [bent_view, truncated_view])
def test_bent_and_truncated_views_are_bounded(maker):
    v = maker()
    before = v.raw()
    rc, got = host_verify(v)
    assert rc == 1
    _same(got[0], np_verify(v)[0], maker.__name__)
    assert got[0]["bad_chains"] + got[0]["list_bad_links"] > 0
    assert host_verify(v, RECLAIM)[0] == ESTATE and v.raw() == before


# ------------------------------------------------------------------------------------------------ reclaim
@pytest.mark.parametrize("n", LEAKS)
def test_reclaim_puts_leaked_entries_back(n):
    v = leaked_view(n)
    ref = v.copy()
    free0 = np_verify(v)[0]["free_entries"]
    assert np_verify(v)[0]["unaccounted"] == n
    rc, got = host_verify(v, RECLAIM)
    wrc, want = np_reclaim(ref)
    assert rc == wrc == 1
    _same(got[0], want[0], n)
    assert got[0]["reclaimed"] == n and got[0]["unaccounted"] == n
    assert got[0]["stray_rows_cleared"] == got[0]["stray_rows"] == sum(1 + i % 2 for i in range(0, n, 3))
    assert v.raw() == ref.raw()  # pool_next, ctl and the entries' bytes
    rc, again = host_verify(v)
    assert rc == 1 and is_clean(again[0]) and again[0]["free_entries"] == free0 + n and again[0]["reclaimed"] == 0
    assert_identities(again[0])
    if n:  # entry r went to list r % 64, behind it the entry 64 ranks on
        assert int(v.tabs[0].heads()[0]) >> 32 == 1 + 1 and (int(v.tabs[0].heads()[min(n, 64) - 1]) & 0xFFFFFFFF) >= 2


@pytest.mark.parametrize("name", "cghi")
def test_reclaim_is_refused_and_writes_nothing(name):
    v, _ = one_change("store", name)
    before = v.raw()
    rc, got = host_verify(v, RECLAIM)
    assert rc == ESTATE and b"nothing reclaimed" in _lib.load().dint_last_error()
    _same(got[0], np_verify(v)[0], name)  # the report is filled all the same
    assert got[0]["reclaimed"] == 0 and v.raw() == before
    assert np_reclaim(v.copy())[0] == ESTATE


def test_a_refusal_in_one_table_keeps_every_table_as_it_was():
    v = sound_view("smallbank")
    t0, t1 = v.tabs
    t0.pool_next[v.meta["lists"][9][0]] = 0       # table 0 leaks five entries ...
    t1.set_u32(1, 52, t1.pool_cap + 7)            # ... table 1 has a bad chain
    before = v.raw()
    rc, got = host_verify(v, RECLAIM)
    assert rc == ESTATE and got[0]["unaccounted"] == 5 and got[0]["reclaimed"] == 0 and got[1]["bad_chains"] == 1 and v.raw() == before


# ------------------------------------------------------------------------------------------------ the view's own check
def test_views_that_fail_the_check():
    L = _lib.load()
    out = (_lib.TableVerify * 5)()

    def rc_of(change, flags=0, cap=5):
        v = sound_view()
        cv = v.c_view()
        change(cv)
        return L.dint_state_verify_view_host(C.byref(cv), out, cap, flags)

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
        assert L.dint_state_verify_view_host(C.byref(cv), out, 5, 0) == EINVAL and b"aligned" in L.dint_last_error()
    assert rc_of(lambda cv: None, cap=0) == EINVAL and b"room for" in L.dint_last_error()
    assert L.dint_state_verify_view_host(None, out, 5, 0) == EINVAL
    assert L.dint_state_verify_view_host(C.byref(v.c_view()), None, 5, 0) == EINVAL


def test_struct_layout_and_flag_name():
    assert C.sizeof(_lib.TableVerify) == 256 and _lib.TableVerify.reclaimed.offset == 16 * 8 and _lib.TableVerify.reserved.offset == 18 * 8
    assert C.sizeof(_lib.TableView) == 56 and C.sizeof(_lib.TablesView) == 16 + 5 * 56
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    abi = open(os.path.join(root, "include", "dint_abi.h")).read()
    assert "#define DINT_VERIFY_RECLAIM 1u" in abi and "#define DINT_ABI_VERSION 5 " in abi
    assert f"#define DINT_VIEW_CTL_BYTES {_lib.VIEW_CTL_BYTES}u" in open(os.path.join(root, "include", "dint_driver.h")).read()


class _FakeEngine:
    def __init__(self, reports):
        self._r = reports

    def state_verify(self):
        return [dict(r) for r in self._r]

    def state_reclaim(self):
        return [dict(r, reclaimed=r["unaccounted"]) for r in self._r]


def test_verify_tables_adds_the_reports_of_a_set():
    a = np_verify(sound_view("smallbank"))
    b = np_verify(one_change("smallbank", "a")[0])
    c = np_verify(one_change("smallbank", "n")[0])
    s = recovery.verify_tables([_FakeEngine(a), _FakeEngine(a)])
    assert s["ok"] and s["clean"] and s["tables"][0]["linked"] == 136 and s["tables"][0]["longest_list"] == 70 and len(s["engines"]) == 2
    s = recovery.verify_tables([_FakeEngine(a), _FakeEngine(b)])
    assert s["ok"] and not s["clean"] and s["tables"][0]["unaccounted"] == 5 and s["tables"][1]["unaccounted"] == 0
    s = recovery.verify_tables([_FakeEngine(c), _FakeEngine(a)])
    assert not s["ok"] and not s["clean"] and s["tables"][0]["stray_rows"] == 1
    assert recovery.verify_tables([_FakeEngine(b)], reclaim=True)["tables"][0]["reclaimed"] == 5
    assert recovery.verify_tables([]) == {"ok": True, "clean": True, "tables": [], "engines": []}


# ------------------------------------------------------------------------------------------------ churn on the host build
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "kv_view_host.cc")
LIB = os.path.join(HERE, "native", "libkv_view_host.so")


@pytest.fixture(scope="module")
def kvh():
    deps = [SRC, os.path.join(HERE, "native", "kv_core_host.cc"), os.path.join(HERE, "..", "dint_amd", "csrc", "dint_kv_core.h")]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", LIB, SRC])
    L = C.CDLL(LIB)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.kvh_create.restype, L.kvh_create.argtypes = vp, [u64, u32, u32]
    L.kvh_destroy.argtypes = [vp]
    L.kvh_insert.argtypes = [vp, u64, u64, vp, u32]
    L.kvh_insert_list.argtypes = [vp, u64, u64, vp, u32, u32]
    L.kvh_delete.argtypes = [vp, u64, u64]
    L.kvh_rotate.argtypes = [vp]
    L.kvh_pool_top.restype, L.kvh_pool_top.argtypes = u32, [vp]
    L.kvh_dump.restype, L.kvh_dump.argtypes = u64, [vp, vp, vp, vp, u64]
    L.kvh_view_fill.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(vp)]
    L.kvh_view_store.argtypes = [vp, vp]
    L.kvh_leak.restype, L.kvh_leak.argtypes = u32, [vp, u32]
    return L


def _kvh_verify(L, h, nb, cap, flags=0):
    """the host build's table as a view (its one pend set is pend set 0); a reclaim's head words go back into the table"""
    ctl = np.zeros(_lib.VIEW_CTL_BYTES, np.uint8)
    ent, nxt = C.c_void_p(), C.c_void_p()
    L.kvh_view_fill(h, ctl.ctypes.data, C.byref(ent), C.byref(nxt))
    v = _lib.TablesView()
    v.workload, v.n_tables, v.shard_index, v.shard_count = int(W.STORE), 1, 0, 1
    tv = v.table[0]
    tv.entries, tv.pool_next, tv.ctl = ent.value, nxt.value, ctl.ctypes.data
    tv.n_local, tv.hash_size, tv.pool_cap, tv.stride, tv.val_size = nb, nb, cap, 256, 40
    out = (_lib.TableVerify * 5)()
    rc = _lib.load().dint_state_verify_view_host(C.byref(v), out, 5, flags)
    assert rc == 1, _lib.load().dint_last_error()
    if flags:
        L.kvh_view_store(h, ctl.ctypes.data)
    return out[0].as_dict(), ctl


def _dump(L, h):
    n = L.kvh_dump(h, None, None, None, 0)
    keys = np.zeros(n, "<u8"); vers = np.zeros(n, "<u4"); vals = np.zeros((n, 40), "u1")
    assert L.kvh_dump(h, keys.ctypes.data, vers.ctypes.data, vals.ctypes.data, n) == n
    return keys.tobytes(), vers.tobytes(), vals.tobytes()


def test_churn_on_the_host_build_stays_clean_and_a_reclaim_is_used_up(kvh):
    L, nb, cap = kvh, 13, 600
    a, b = L.kvh_create(nb, cap, 40), L.kvh_create(nb, cap, 40)
    rng = np.random.default_rng(11)
    pool = (np.arange(1, 401, dtype=np.uint64) * np.uint64(7919)).tolist()
    bucket = dict(zip(pool, np_bucket(pool, nb).astype(np.int64).tolist()))
    live, val = set(), np.zeros(40, np.uint8)
    checks = pending_seen = 0
    for step in range(6000):
        k = pool[int(rng.integers(len(pool)))]
        val[0] = step & 0xFF
        for h in (a, b):
            if k in live:
                assert L.kvh_delete(h, bucket[k], k) == 0
            else:
                assert L.kvh_insert(h, bucket[k], k, val.ctypes.data, step) == 0
        live ^= {k}
        if step % 97 == 0:
            L.kvh_rotate(a); L.kvh_rotate(b)
        if step % 750 == 749:
            r, _ = _kvh_verify(L, a, nb, cap)
            assert is_clean(r) and r["rows"] == len(live) and r["pool_top"] == L.kvh_pool_top(a), r
            assert_identities(r)
            checks += 1
            pending_seen += r["pending_entries"] + r["free_entries"]
    assert checks == 8 and pending_seen > 0  # entries were freed and recycled, or the churn checks nothing
    # leak ten entries by hand: handed out and never linked
    assert L.kvh_leak(a, 10) == 10
    r, _ = _kvh_verify(L, a, nb, cap)
    assert r["unaccounted"] == 10 and r["stray_rows"] == r["stray_valid_entries"] == 10 and all(r[k] == 0 for k in REFUSING)
    r, _ = _kvh_verify(L, a, nb, cap, RECLAIM)
    assert r["reclaimed"] == 10 and r["stray_rows_cleared"] == 10
    r, ctl = _kvh_verify(L, a, nb, cap)
    assert is_clean(r), r
    assert _dump(L, a) == _dump(L, b)
    # go on inserting beside the twin: a list that holds a reclaimed entry is popped before pool_top moves
    fresh = (np.arange(1, 4000, dtype=np.uint64) * np.uint64(104729) + np.uint64(5)).tolist()
    fb = np_bucket(fresh, nb).astype(np.int64).tolist()
    used_up = grew = 0
    for i, (k, kb) in enumerate(zip(fresh, fb)):
        heads = _kvh_verify(L, a, nb, cap)[1][64:64 + 8 * NLISTS].view("<u8") & 0xFFFFFFFF
        full = [l for l in range(10) if heads[l]]  # entry r of the ten went to free list r
        used_up = 10 - len(full)
        if used_up == 10 and grew:
            break
        lst = full[i % len(full)] if full else 0
        top = L.kvh_pool_top(a)
        assert L.kvh_insert_list(a, kb, k, val.ctypes.data, 0, lst) == 0 and L.kvh_insert_list(b, kb, k, val.ctypes.data, 0, lst) == 0
        if L.kvh_pool_top(a) > top:
            assert not full, "pool_top grew although the list held an entry"
            grew += 1
    assert used_up == 10 and grew, "the reclaimed entries were never used up"
    r, _ = _kvh_verify(L, a, nb, cap)
    assert is_clean(r), r
    assert _dump(L, a) == _dump(L, b)
    L.kvh_destroy(a); L.kvh_destroy(b)


# ------------------------------------------------------------------------------------------------ the fixtures as a file
def all_cases():
    """(name, view, flags): everything above that the device and the stand-alone program are shown as well"""
    c = [(f"sound_{k}", sound_view(k), 0) for k in KINDS]
    c += [(f"{k}_{n}", one_change(k, n)[0], 0) for k in KINDS for n in CHANGES]
    c += [("bent", bent_view(), 0), ("truncated", truncated_view(), 0)]
    c += [(f"reclaim_{n}", leaked_view(n), RECLAIM) for n in LEAKS]
    c += [(f"refused_{n}", one_change("store", n)[0], RECLAIM) for n in "cghi"] + [("refused_bent", bent_view(), RECLAIM)]
    return c


def expected(view, flags):
    """(rc, reports, the view afterwards) by the numpy form"""
    after = view.copy()
    if flags & RECLAIM:
        rc, rep = np_reclaim(after)
    else:
        rc, rep = len(view.tabs), np_verify(after)
    return rc, rep, after


if __name__ == "__main__":
    # u64 cases; per case: i32 {workload, n_tables, shard_index, shard_count, flags, rc}; per table u64 {n_local, hash_size, pool_cap,
    # stride, val_size}, entries, pool_next, ctl; then per table the numpy report as 32 u64; then per table entries, pool_next, ctl
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
                f.write(struct.pack("<32Q", *([r[k] for k in FIELDS] + [0] * 14)))
            for t in after.tabs:
                f.write(t.entries.tobytes() + t.pool_next.tobytes() + t.ctl.tobytes())
    print(len(cases), "views")
