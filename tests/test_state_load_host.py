"""The bulk load's rule on the host (dint_amd/csrc/state_load.h): dint_state_load_place_host over caller-described tables that hold
nothing against the serial kv_insert<kv_host_mem> of the same rows in order (tests/native/kv_core_host.cc, the code the request
path runs), dint_populate_rows_host and the tile tables against themselves at other tilings, and the stand-alone sanitizer program
tests/native/state_load_main.cc, which holds the rule to kv_insert and to dint_pop::generate.  No device call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from dint_amd import _lib, wire
from kvkeys import keys_by_bucket, np_bucket, overflow_need

W = wire.Workload
EINVAL, ENOMEM, ESTATE = -1, -2, -5
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "kv_core_host.cc")
LIB = os.path.join(HERE, "native", "libkv_core_host.so")
PER = [0, 1, 4, 5, 8, 9, 41]


@pytest.fixture(scope="module")
def kvh():
    hdr = os.path.join(HERE, "..", "dint_amd", "csrc", "dint_kv_core.h")
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", LIB, SRC])
    L = C.CDLL(LIB)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.kvh_create.restype, L.kvh_create.argtypes = vp, [u64, u32, u32]
    L.kvh_destroy.argtypes = [vp]
    L.kvh_get.argtypes = [vp, u64, u64, vp, vp]
    L.kvh_insert.argtypes = [vp, u64, u64, vp, u32]
    L.kvh_pool_top.restype, L.kvh_pool_top.argtypes = u32, [vp]
    L.kvh_dump.restype, L.kvh_dump.argtypes = u64, [vp, vp, vp, vp, u64]
    return L


class View:
    """one table of a store (40-byte values) or smallbank (8) view that holds nothing, in numpy memory"""

    def __init__(self, hash_size, pool_cap, vs=40, shard=(0, 1)):
        self.vs, self.stride, self.shard = vs, 256 if vs == 40 else 128, shard
        self.n_local = -(-hash_size // shard[1])
        self.pool_cap = pool_cap
        raw = np.zeros((self.n_local + pool_cap) * self.stride + 16, np.uint8)
        off = -raw.ctypes.data % 16
        self.entries = raw[off:off + (self.n_local + pool_cap) * self.stride]
        self.pool_next = np.zeros(max(pool_cap, 1), np.uint32)
        self.ctl = np.zeros(_lib.VIEW_CTL_BYTES // 8, np.uint64)
        wl = W.STORE if vs == 40 else W.SMALLBANK
        v = self.v = _lib.TablesView()
        v.workload, v.n_tables, v.shard_index, v.shard_count = int(wl), 1 if vs == 40 else 2, shard[0], shard[1]
        for t in range(v.n_tables):  # (smallbank: the second table is a second description of the same memory, never loaded)
            tv = v.table[t]
            tv.entries, tv.pool_next, tv.ctl = self.entries.ctypes.data, self.pool_next.ctypes.data, self.ctl.ctypes.data
            tv.n_local, tv.hash_size, tv.pool_cap, tv.stride, tv.val_size = self.n_local, hash_size, pool_cap, self.stride, vs

    def load(self, keys, vers, vals):
        keys = np.ascontiguousarray(keys, "<u8")
        vals = np.ascontiguousarray(vals, "u1")
        s = _lib.LoadStats()
        rc = _lib.load().dint_state_load_place_host(C.byref(self.v), 0, keys.ctypes.data, None if vers is None else vers.ctypes.data,
                                                    vals.ctypes.data, len(keys), C.byref(s))
        return rc, s

    def pool_top(self):
        return int(self.ctl.view(np.uint32)[0])

    def walk(self):
        """per local bucket the entries of the chain as (is_inline, validw), and the rows in chain order"""
        shape, keys, vers, vals = [], [], [], []
        e = self.entries.reshape(-1, self.stride)
        for b in range(self.n_local):
            cur = int(e[b, 56:60].view("<u4")[0])
            sh = []
            while cur:
                row = e[b if cur == 1 else self.n_local + cur - 2]
                vw = row[48:52]
                sh.append((cur == 1, int(vw.view("<u4")[0])))
                for i in range(4):
                    if vw[i]:
                        keys.append(int(row[8 * i:8 * i + 8].view("<u8")[0]))
                        vers.append(int(row[32 + 4 * i:36 + 4 * i].view("<u4")[0]))
                        vals.append(row[64 + i * self.vs:64 + (i + 1) * self.vs].tobytes())
                cur = int(row[52:56].view("<u4")[0])
                assert len(sh) <= 4096
            shape.append(sh)
        return shape, keys, vers, vals


def rows_for(hash_size, per, seed, dup_in=None):
    """keys with per[b] of them in global bucket b, in an order that mixes the buckets; versions and values that name the row"""
    keys = keys_by_bucket(hash_size, per, seed=seed)
    keys = keys[np.random.default_rng(seed).permutation(len(keys))]
    if dup_in is not None:  # rows 3 and 4 of bucket dup_in share a key: the pair straddles the entry boundary
        at = np.nonzero(np_bucket(keys, hash_size) == np.uint64(dup_in))[0]
        keys[at[4]] = keys[at[3]]
    vers = (np.arange(len(keys)) + 500).astype("<u4")
    return keys, vers


def vals_for(n, vs):
    return ((np.arange(n)[:, None] * 3 + np.arange(vs)[None, :]) % 251).astype(np.uint8)


def serial(kvh, keys, vers, vals, hash_size, pool_cap, vs, shard=(0, 1)):
    """the same rows through kv_insert, one by one: (dump, pool_top, handle)"""
    n_local = -(-hash_size // shard[1])
    h = kvh.kvh_create(n_local, pool_cap, vs)
    g = np_bucket(keys, hash_size).astype(np.int64)
    for i in np.nonzero(g % shard[1] == shard[0])[0]:
        assert kvh.kvh_insert(h, int(g[i] // shard[1]), int(keys[i]), vals[i].ctypes.data, int(vers[i])) == 0
    n = kvh.kvh_dump(h, None, None, None, 0)
    k = np.zeros(n, "<u8"); v = np.zeros(n, "<u4"); x = np.zeros((n, vs), "u1")
    kvh.kvh_dump(h, k.ctypes.data, v.ctypes.data, x.ctypes.data, n)
    return (k, v, x), kvh.kvh_pool_top(h), h


@pytest.mark.parametrize("vs", [40, 8])
@pytest.mark.parametrize("dup", [None, 4, 6])
def test_placement_equals_the_serial_load(kvh, vs, dup):
    keys, vers = rows_for(7, PER, seed=3 + vs, dup_in=dup)
    vals = vals_for(len(keys), vs)
    need = overflow_need(PER)
    view = View(7, need, vs)  # (the pool fits exactly)
    rc, s = view.load(keys, vers, vals)
    assert rc == 0, _lib.load().dint_last_error()
    (k, v, x), top, h = serial(kvh, keys, vers, vals, 7, need, vs)
    try:
        shape, wk, wv, wx = view.walk()
        assert wk == k.tolist() and wv == v.tolist() and b"".join(wx) == x.tobytes()
        assert view.pool_top() == top == need
        # inline entry last (the oldest), full entries behind the newest, which holds the remainder
        for b, r in enumerate(PER):
            ent = -(-r // 4)
            assert len(shape[b]) == ent
            if ent:
                assert [i for i, _ in shape[b]] == [False] * (ent - 1) + [True]
                assert shape[b][0][1] == 0x01010101 >> (8 * (4 * ent - r)) and all(w == 0x01010101 for _, w in shape[b][1:])
        assert (s.rows_loaded, s.foreign_rows, s.direct) == (len(keys), 0, 1)
        assert (s.table[0].overflow_entries, s.table[0].longest_chain_entries, s.table[0].rows) == (need, 11, len(keys))
        if dup is not None:  # the visible row is the one the serial load shows: the LATER one, first slot of the newer entry
            at = np.nonzero(keys == keys[np.nonzero(np_bucket(keys, 7) == np.uint64(dup))[0][3]])[0]
            got = np.zeros(vs, np.uint8); ver = C.c_uint32()
            assert len(at) == 2 and kvh.kvh_get(h, dup, int(keys[at[0]]), got.ctypes.data, C.byref(ver)) == 0
            assert ver.value == vers[at[1]] and wv[wk.index(int(keys[at[0]]))] == vers[at[1]]
    finally:
        kvh.kvh_destroy(h)


def test_placement_without_versions_and_with_no_rows():
    keys, _ = rows_for(7, PER, seed=9)
    view = View(7, 64)
    rc, s = view.load(keys, None, vals_for(len(keys), 40))
    assert rc == 0 and set(view.walk()[2]) == {0}
    empty = View(7, 0)
    rc, s = empty.load(np.zeros(0, "<u8"), None, np.zeros((0, 40), "u1"))
    assert rc == 0 and s.rows_loaded == 0 and not empty.entries.any()


@pytest.mark.parametrize("index", [0, 1, 2])
def test_three_shards_keep_their_home_rows(kvh, index):
    hs = 21
    keys, vers = rows_for(hs, PER * 3, seed=5, dup_in={0: 6, 1: 13, 2: 20}[index])  # (a 41-row bucket that is home to shard index)
    vals = vals_for(len(keys), 40)
    g = np_bucket(keys, hs).astype(np.int64)
    home = g % 3 == index
    need = overflow_need(np.bincount(g[home] // 3, minlength=7))
    view = View(hs, need, 40, shard=(index, 3))
    rc, s = view.load(keys, vers, vals)
    assert rc == 0, _lib.load().dint_last_error()
    (k, v, x), top, h = serial(kvh, keys, vers, vals, hs, need, 40, shard=(index, 3))
    kvh.kvh_destroy(h)
    _, wk, wv, wx = view.walk()
    assert wk == k.tolist() and wv == v.tolist() and b"".join(wx) == x.tobytes() and view.pool_top() == top == need
    assert (s.rows_loaded, s.foreign_rows) == (int(home.sum()), int((~home).sum()))


def test_a_pool_one_entry_short_is_refused_with_the_need_and_nothing_written():
    keys, vers = rows_for(7, PER, seed=2)
    need = overflow_need(PER)
    view = View(7, need - 1)
    view.entries[:] = 0  # (what a table that holds nothing is)
    before = (view.entries.copy(), view.ctl.copy(), view.pool_next.copy())
    rc, s = view.load(keys, vers, vals_for(len(keys), 40))
    assert rc == ENOMEM and s.table[0].overflow_entries == need and s.direct == 0
    assert (view.entries == before[0]).all() and (view.ctl == before[1]).all() and (view.pool_next == before[2]).all()
    # a bucket beyond 4096 entries: refused as well, nothing written
    one = np.full(4 * 4096 + 1, 77, "<u8")
    big = View(1, 5000)
    rc, s = big.load(one, None, np.zeros((len(one), 40), "u1"))
    assert rc == ESTATE and not big.entries.any() and big.pool_top() == 0
    rc, s = big.load(one[:-1], None, np.zeros((len(one) - 1, 40), "u1"))
    assert rc == 0 and big.pool_top() == 4095 and s.table[0].longest_chain_entries == 4096


def test_bad_arguments_are_refused():
    view = View(7, 4)
    k = np.ones(3, "<u8"); x = np.zeros((3, 40), "u1")
    L = _lib.load()
    s = _lib.LoadStats()
    assert L.dint_state_load_place_host(C.byref(view.v), 1, k.ctypes.data, None, x.ctypes.data, 3, C.byref(s)) == EINVAL  # store has one table
    assert L.dint_state_load_place_host(C.byref(view.v), 0, None, None, x.ctypes.data, 3, C.byref(s)) == EINVAL
    assert L.dint_state_load_place_host(C.byref(view.v), 0, k.ctypes.data, None, None, 3, C.byref(s)) == EINVAL
    assert L.dint_state_load_place_host(None, 0, k.ctypes.data, None, x.ctypes.data, 3, C.byref(s)) == EINVAL
    assert not view.entries.any()


# ---- generation ----------------------------------------------------------------------------------------------------------
TABLES = [(W.STORE, 0), (W.SMALLBANK, 0), (W.SMALLBANK, 1)] + [(W.TATP, t) for t in range(5)]


def rows_host(wl, table, first, count):
    L = _lib.load()
    vs = 8 if wl == W.SMALLBANK else 40
    n = L.dint_populate_rows_host(int(wl), table, first, count, None, None, 0)
    assert n >= 0
    keys = np.zeros(n, "<u8"); vals = np.zeros((n, vs), "u1")
    assert L.dint_populate_rows_host(int(wl), table, first, count, keys.ctypes.data, vals.ctypes.data, n) == n
    return keys, vals


@pytest.mark.parametrize("wl,table", TABLES)
def test_the_rows_of_a_range_do_not_depend_on_how_it_is_cut(wl, table):
    tile = _lib.load().dint_populate_tile()
    assert tile == 256
    for n in (1, tile - 1, tile, tile + 1, 3 * tile + 7):
        wk, wv = rows_host(wl, table, 0, n)
        parts = [rows_host(wl, table, f, min(tile, n - f)) for f in range(0, n, tile)]
        assert (np.concatenate([p[0] for p in parts]) == wk).all() and (np.concatenate([p[1] for p in parts]) == wv).all()
        odd = [rows_host(wl, table, f, min(97, n - f)) for f in range(0, n, 97)]
        assert (np.concatenate([p[0] for p in odd]) == wk).all() and (np.concatenate([p[1] for p in odd]) == wv).all()
        assert len(wk) > 0


def test_row_shapes_of_the_population():
    """what SURVEY / dint_populate.h say about the rows, on the rule's output"""
    k, v = rows_host(W.STORE, 0, 5, 2)
    assert len(k) == 24 and (k & np.uint64(0xFFFFFFFF)).tolist() == [5] * 12 + [6] * 12 and (v[:, 1] == 0x5a).all()
    assert ((v[:, 0] >= 1) & (v[:, 0] <= 24)).all() and not v[:, 2:].any()
    k, v = rows_host(W.SMALLBANK, 1, 9, 3)
    assert k.tolist() == [9, 10, 11] and (v.view("<u4")[:, 0] == 98).all() and (v.view("<f4")[:, 1] == 1e9).all()
    k, v = rows_host(W.TATP, 1, 123456789, 1)
    assert k.tolist() == [0x123456789] and v[0, :4].view("<u4")[0] == 123456789 and v[0, 4] == 98
    k, v = rows_host(W.TATP, 2, 0, 500)
    ty = (k >> np.uint64(32)).astype(np.int64)
    assert ((ty >= 1) & (ty <= 4)).all() and (v[:, 0] == 99).all() and len(np.unique(k)) == len(k)
    per = np.bincount((k & np.uint64(0xFFFFFFFF)).astype(np.int64), minlength=500)
    assert per.min() >= 1 and per.max() <= 4
    kc, vc = rows_host(W.TATP, 4, 0, 500)
    ks, _ = rows_host(W.TATP, 3, 0, 500)
    assert np.isin(kc & np.uint64(0xFFFFFFFFFF), ks).all() and (vc[:, 1] == 101).all()  # every CALL FORWARDING row has its SPECIAL FACILITY


def test_tile_tables_are_a_prefix_property():
    L = _lib.load()
    tile = L.dint_populate_tile()
    for table, other in ((2, None), (3, 4), (4, 3)):
        n = 9 * tile + 5
        st = np.zeros(10, "<u8"); ro = np.zeros(10, "<u8")
        assert L.dint_populate_tile_states_host(int(W.TATP), table, n, st.ctypes.data, ro.ctypes.data, 10) == 10
        s2 = np.zeros(4, "<u8"); r2 = np.zeros(4, "<u8")
        assert L.dint_populate_tile_states_host(int(W.TATP), table, 3 * tile, s2.ctypes.data, r2.ctypes.data, 4) == 4
        assert (s2 == st[:4]).all() and (r2 == ro[:4]).all() and st[0] == 0xdeadbeef and ro[0] == 0
        for k in (1, 4, 9):  # rows before tile k = the rows of the subscribers before it
            assert len(rows_host(W.TATP, table, 0, k * tile)[0]) == ro[k]
        if other is not None:  # one stream fills both tables: the states are the same
            so = np.zeros(10, "<u8")
            assert L.dint_populate_tile_states_host(int(W.TATP), other, n, so.ctypes.data, None, 10) == 10 and (so == st).all()
    assert L.dint_populate_tile_states_host(int(W.TATP), 0, 100, None, None, 0) == ESTATE
    assert L.dint_populate_tile_states_host(int(W.STORE), 3, 100, None, None, 0) == EINVAL
    assert L.dint_populate_rows_host(int(W.FASST), 0, 0, 1, None, None, 0) == EINVAL


def test_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    """tests/native/state_load_main.cc -- the rule against kv_insert and against dint_pop::generate, with a main of its own --
    built with -fsanitize=address,undefined and run as it is"""
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    exe = str(tmp_path / "state_load_main")
    subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas"] + san + [os.path.join(HERE, "native", "state_load_main.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and not r.stderr, (r.stdout[-400:], r.stderr[-2000:])
