"""The HBM table layout (dint_amd/csrc/dint_kv_core.h: inline entry + overflow pool, chain head in
the inline header) compiled for the host and driven op by op against the oracle's chained kvs
(store/udp/kvs.h semantics).  Same source the HIP kernels run; catches chain-order, prepend,
free/unlink, pool-recycling and duplicate-key bugs without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "kv_core_host.cc")
LIB = os.path.join(HERE, "native", "libkv_core_host.so")


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
    L.kvh_set.argtypes = [vp, u64, u64, vp]
    L.kvh_insert.argtypes = [vp, u64, u64, vp, u32]
    L.kvh_delete.argtypes = [vp, u64, u64]
    L.kvh_rotate.argtypes = [vp]
    L.kvh_pool_top.restype, L.kvh_pool_top.argtypes = u32, [vp]
    L.kvh_listed.restype, L.kvh_listed.argtypes = u32, [vp, C.c_int]
    L.kvh_set_lock_bytes.argtypes = [vp, u64, u32]
    L.kvh_get_lock_bytes.restype, L.kvh_get_lock_bytes.argtypes = u32, [vp, u64]
    L.kvh_dump.restype, L.kvh_dump.argtypes = u64, [vp, vp, vp, vp, u64]
    return L


def bucket_of(key, nb):
    return orc.fasthash64(int(key).to_bytes(8, "little")) % nb


def dump(L, h, vs):
    n = L.kvh_dump(h, None, None, None, 0)
    keys = np.zeros(n, "<u8"); vers = np.zeros(n, "<u4"); vals = np.zeros((n, vs), "u1")
    assert L.kvh_dump(h, keys.ctypes.data, vers.ctypes.data, vals.ctypes.data, n) == n
    return keys, vers, vals


@pytest.mark.parametrize("vs,nb,nkeys,nops,seed,dups", [
    (40, 1, 30, 4000, 1, False), (40, 3, 60, 8000, 2, False), (8, 2, 40, 6000, 3, False),
    (40, 2, 24, 6000, 4, True), (8, 1, 12, 5000, 5, True), (40, 7, 200, 20000, 6, False),
])
def test_layout_matches_chained_kvs(kvh, vs, nb, nkeys, nops, seed, dups):
    """Random get/set/insert/delete; with dups=True inserts of existing keys create duplicate rows,
    which only an exact chain-order reproduction answers the same way as the reference."""
    L = kvh
    rng = np.random.default_rng(seed)
    h = L.kvh_create(nb, 4096 if dups else 64, vs)  # duplicate rows pile up: inserts outnumber deletes
    o = orc.KvsOracle(nb, vs)
    keys = rng.integers(1, 2**62, nkeys, dtype=np.uint64)
    live = {}
    for b in range(nb):
        L.kvh_set_lock_bytes(h, b, 0xA5000000 | b)
    try:
        for step in range(nops):
            k = int(keys[rng.integers(0, nkeys)])
            b = bucket_of(k, nb)
            op = rng.integers(0, 10)
            val = rng.integers(0, 256, vs, dtype=np.uint8)
            if op < 3:
                ov, over = o.get(k)
                gv = np.zeros(vs, "u1"); gver = C.c_uint32(0xDEAD)
                rc = L.kvh_get(h, b, k, gv.ctypes.data, C.addressof(gver))
                assert (rc == 1) == (ov is None)
                if ov is not None:
                    assert (gv == ov).all() and gver.value == over
            elif op < 5:
                assert L.kvh_set(h, b, k, val.ctypes.data) == o.set(k, val)
            elif op < 8:
                if not dups and live.get(k, 0) > 0:
                    continue
                o.insert(k, val)
                assert L.kvh_insert(h, b, k, val.ctypes.data, 0) == 0
                live[k] = live.get(k, 0) + 1
            else:
                rc = o.delete(k)
                assert L.kvh_delete(h, b, k) == rc
                if rc == 0:
                    live[k] -= 1
            if step % 97 == 0:
                L.kvh_rotate(h)  # a pass boundary: freed overflow entries become reusable
            if step % 500 == 0:
                a, bb = dump(L, h, vs), o.dump()
                assert all((x == y).all() for x, y in zip(a, bb)), step
        a, bb = dump(L, h, vs), o.dump()
        assert all((x == y).all() for x, y in zip(a, bb))
        for b in range(nb):  # lock bytes live in the inline header next to `head`: never clobbered
            assert L.kvh_get_lock_bytes(h, b) == (0xA5000000 | b)
        # recycling keeps the pool bounded: far fewer bump allocations than overflow inserts
        assert L.kvh_pool_top(h) <= (4096 if dups else 64)
    finally:
        L.kvh_destroy(h)


def test_pool_exhaustion_is_reported(kvh):
    L = kvh
    h = L.kvh_create(1, 2, 40)
    val = np.zeros(40, "u1")
    ok = [L.kvh_insert(h, 0, 100 + i, val.ctypes.data, 0) for i in range(16)]
    assert ok[:12] == [0] * 12 and ok[12:] == [1] * 4  # inline + 2 pool entries = 12 rows
    assert dump(L, h, 40)[0].size == 12
    L.kvh_destroy(h)


@pytest.mark.parametrize("vs,nb,nkeys,pool,nops,seed,dups", [
    (40, 1, 40, 2, 6000, 1, False), (40, 3, 90, 5, 9000, 2, False), (8, 2, 120, 9, 9000, 3, False),
    (40, 2, 24, 5, 6000, 4, True), (8, 1, 12, 9, 5000, 5, True), (40, 7, 400, 9, 20000, 6, False),
])
def test_overrun_pool_refuses_and_stays_exact(kvh, vs, nb, nkeys, pool, nops, seed, dups):
    """Pools of 2, 5 and 9 entries that the op stream overruns, a rotation every 97 steps.  A refused insert stores nothing: it
    is skipped on the oracle and everything else agrees at every step, the dump included.  An insert is refused only when the
    bump allocator is at pool_cap and no entry is poppable, and however many inserts fail the counter stays at pool_cap (the
    clamp in kv_pool_alloc).  tests/native/kv_core_pool_main.cc is the same walk as a stand-alone program for the sanitizers."""
    L = kvh
    rng = np.random.default_rng(seed)
    h = L.kvh_create(nb, pool, vs)
    o = orc.KvsOracle(nb, vs)
    keys = rng.integers(1, 2**62, nkeys, dtype=np.uint64)
    live, refused, stored = {}, 0, 0
    try:
        for step in range(nops):
            k = int(keys[rng.integers(0, nkeys)])
            b = bucket_of(k, nb)
            op = rng.integers(0, 10)
            val = rng.integers(0, 256, vs, dtype=np.uint8)
            if op < 3:
                ov, over = o.get(k)
                gv = np.zeros(vs, "u1"); gver = C.c_uint32(0xDEAD)
                rc = L.kvh_get(h, b, k, gv.ctypes.data, C.addressof(gver))
                assert (rc == 1) == (ov is None)
                if ov is not None:
                    assert (gv == ov).all() and gver.value == over
            elif op < 5:
                assert L.kvh_set(h, b, k, val.ctypes.data) == o.set(k, val)
            elif op < 8:
                if not dups and live.get(k, 0) > 0:
                    continue
                top, poppable = L.kvh_pool_top(h), L.kvh_listed(h, 0)
                if L.kvh_insert(h, b, k, val.ctypes.data, 0) == 0:
                    o.insert(k, val)
                    live[k] = live.get(k, 0) + 1
                    stored += 1
                else:
                    assert top == pool and poppable == 0, step
                    refused += 1
                assert L.kvh_pool_top(h) <= pool and (not refused or L.kvh_pool_top(h) == pool), step
            else:
                rc = o.delete(k)
                assert L.kvh_delete(h, b, k) == rc
                if rc == 0:
                    live[k] -= 1
            if step % 97 == 0:
                L.kvh_rotate(h)
            if step % 500 == 0:
                a, bb = dump(L, h, vs), o.dump()
                assert all(x.shape == y.shape and (x == y).all() for x, y in zip(a, bb)), step
        a, bb = dump(L, h, vs), o.dump()
        assert all(x.shape == y.shape and (x == y).all() for x, y in zip(a, bb))
        assert refused > 0 and stored > 0  # or the case is void
        assert L.kvh_listed(h, 0) + L.kvh_listed(h, 1) <= pool
    finally:
        L.kvh_destroy(h)


# ---- the key helpers of the pool tests (tests/kvkeys.py) ----------------------------------------------------------------
def test_keys_by_bucket_gives_exact_counts_and_well_formed_keys():
    import kvkeys

    counts = [0, 1, 4, 5, 8, 9, 3, 0, 12, 13, 2]
    keys = kvkeys.keys_by_bucket(len(counts), counts, seed=4)
    assert len(np.unique(keys)) == len(keys) == sum(counts)
    b = [bucket_of(k, len(counts)) for k in keys]
    assert b == sorted(b) and np.bincount(b, minlength=len(counts)).tolist() == counts  # bucket order, exactly that many
    assert (kvkeys.np_bucket(keys, len(counts)).astype(np.int64) == np.array(b)).all()
    assert kvkeys.overflow_need(counts) == 0 + 0 + 0 + 1 + 1 + 2 + 0 + 0 + 2 + 3 + 0
    cf = kvkeys.keys_by_bucket(37, 5, seed=2, key_of=kvkeys.cf_key_of).reshape(37, 5)
    assert len(np.unique(cf)) == cf.size and all(bucket_of(k, 37) == g for g in range(37) for k in cf[g])
    sf, st = (cf >> np.uint64(32)) & np.uint64(0xFF), cf >> np.uint64(40)
    assert ((sf >= 1) & (sf <= 4)).all() and np.isin(st, [0, 8, 16]).all()  # s_id | sf_type << 32 | start_time << 40


def test_overflow_need_is_what_an_insert_only_table_links(kvh):
    import kvkeys

    counts = [0, 3, 4, 5, 8, 9, 17]
    keys = kvkeys.keys_by_bucket(len(counts), counts, seed=6)
    need = kvkeys.overflow_need(counts)
    h = kvh.kvh_create(len(counts), need, 40)  # an exact fit
    val = np.zeros(40, "u1")
    try:
        assert all(kvh.kvh_insert(h, bucket_of(k, len(counts)), int(k), val.ctypes.data, 0) == 0 for k in keys)
        assert kvh.kvh_pool_top(h) == need
        extra = kvkeys.keys_by_bucket(len(counts), [0, 0, 1, 0, 1, 0, 0], seed=7)  # into the two buckets whose last entry is full
        assert [kvh.kvh_insert(h, bucket_of(k, len(counts)), int(k), val.ctypes.data, 0) for k in extra] == [1, 1]
        assert kvh.kvh_pool_top(h) == need and dump(kvh, h, 40)[0].size == sum(counts)
    finally:
        kvh.kvh_destroy(h)


@pytest.mark.parametrize("kind", ["issue", "crossing"])
@pytest.mark.parametrize("wl", ["store", "tatp"])
def test_churn_case_sizes_refuse_some_inserts_but_fewer_than_half(kvh, wl, kind):
    """The sizes of the churn case of tests/test_gpu_kv_pool.py on the host build: every table of the populated server with the
    case's pool_entries (kvkeys.churn_pool), the trace's INSERTs and DELETEs in order, a rotation at every pass boundary.
    0 < refused < half the INSERTs -- deletes (tatp) and free slots keep most inserts going.  The "crossing" size really
    crosses: on every table that refuses, pool_top + the INSERTs of the pass fits the pool in pass 0 (the engine takes its closed
    forms) and exceeds it in a later pass (it stops taking them), before the first refusal."""
    import kvkeys
    from dint_amd import wire

    W = wire.Workload
    wl = W.STORE if wl == "store" else W.TATP
    passes = kvkeys.churn_trace(wl, kind)
    pool = kvkeys.churn_pool(wl, passes, kind)
    o = kvkeys.churn_oracle(wl)
    nt = kvkeys.N_TABLES[wl]
    hs = [kvkeys.CHURN_SUBS[wl] * 18 // 4] if wl == W.STORE else [o.hash_size(t) for t in range(nt)]
    tabs = [kvh.kvh_create(hs[t], pool, 40) for t in range(nt)]
    val = np.zeros(40, "u1")
    try:
        for t in range(nt):
            keys = o.dump()[0] if wl == W.STORE else o.dump(t)[0]
            for k, b in zip(keys.tolist(), kvkeys.np_bucket(keys, hs[t]).tolist()):
                assert kvh.kvh_insert(tabs[t], b, k, val.ctypes.data, 0) == 0  # the population fits
        ins_types, del_types = kvkeys.INSERT_TYPES[wl], (() if wl == W.STORE else (22, 23))
        n_ins = 0
        refused = [[0] * nt for _ in passes]     # [pass][table]
        fits = [[True] * nt for _ in passes]     # pool_top + the pass's INSERTs <= pool_cap at the start of the pass
        for p, m in enumerate(passes):
            for t, c in enumerate(kvkeys.pass_inserts(wl, m)):
                fits[p][t] = kvh.kvh_pool_top(tabs[t]) + c <= pool
            sel = np.isin(m["type"], ins_types + del_types)
            tb = m["table"][sel].tolist() if wl == W.TATP else [0] * int(sel.sum())
            keys = m["key"][sel]
            bk = np.zeros(len(keys), np.int64)
            for t in range(nt):
                mt = np.array(tb) == t
                bk[mt] = kvkeys.np_bucket(keys[mt], hs[t]).astype(np.int64)
            for ty, t, k, b in zip(m["type"][sel].tolist(), tb, keys.tolist(), bk.tolist()):
                if ty in ins_types:
                    n_ins += 1
                    refused[p][t] += kvh.kvh_insert(tabs[t], b, k, val.ctypes.data, 0)
                else:
                    kvh.kvh_delete(tabs[t], b, k)
            for h in tabs:
                kvh.kvh_rotate(h)
        total = sum(map(sum, refused))
        assert 0 < total < n_ins // 2, (pool, n_ins, total)
        for t in range(nt):
            first = next((p for p in range(len(passes)) if refused[p][t]), None)
            if first is None:
                continue
            low = [p for p in range(len(passes)) if not fits[p][t]]
            if kind == "crossing":
                assert pool > 4096 or wl == W.TATP, pool
                assert fits[0][t] and low and 0 < low[0] <= first, (t, pool, low[:3], first)
            else:
                assert low[0] == 0, (t, pool, low[:3], first)  # (churn_pool: always request by request)
    finally:
        for h in tabs:
            kvh.kvh_destroy(h)


def test_stand_alone_pool_program_runs_clean_under_the_sanitizers(tmp_path):
    """tests/native/kv_core_pool_main.cc -- the overrun-pool walk with a main of its own -- built with
    -fsanitize=address,undefined together with the oracle's C file, and run as it is"""
    root = os.path.join(HERE, "..")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    obj, exe = str(tmp_path / "dint_oracle.o"), str(tmp_path / "kv_core_pool")
    subprocess.check_call(["gcc", "-c"] + san + [os.path.join(root, "oracle", "dint_oracle.c"), "-o", obj])
    subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas"] + san + [os.path.join(HERE, "native", "kv_core_pool_main.cc"), obj, "-o", exe, "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and not r.stderr, (r.stdout[-400:], r.stderr[-2000:])
