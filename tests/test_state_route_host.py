"""The record routing's rule on the host (dint_amd/csrc/state_route.h through dint_records_route_host, include/dint_driver.h) against
numpy: a stable argsort by home, the home from tests/kvkeys.py np_bucket -- a vectorised fasthash64 that shares no code with the
rule -- and the bucket counts from the formulas the reference's servers use.  Every comparison is exact.  No device call."""
import os
import re

import numpy as np
import pytest

from dint_amd import _lib, wire
from kvkeys import np_bucket

W = wire.Workload
EINVAL, ESTATE = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(W.TATP, 300), (W.SMALLBANK, 1000), (W.STORE, 1000)]
HS = [1, 2, 3, 5, 64, 255]


def hash_sizes(wl, n):
    """store/udp/server.cc:112-114, tatp/udp/server_shard.cc:75-79, smallbank/udp/server_shard.cc:75-76"""
    if wl == W.STORE:
        return [n * 18 // 4]
    if wl == W.TATP:
        return [n * 3 // 2 // 4] * 2 + [n * 15 // 4 // 4] * 2 + [n * 45 // 8 // 4]
    return [n * 3 // 2 // 4] * 2


def np_home(rec, wl, n_rows, H):
    """(fasthash64(key) % hash_size[table]) % H per record"""
    hs = hash_sizes(wl, n_rows)
    home = np.zeros(len(rec), np.int64)
    for t, h in enumerate(hs):
        m = rec["table"] == t
        home[m] = (np_bucket(rec["key"][m], h) % np.uint64(H)).astype(np.int64)
    return home


def np_route(rec, wl, n_rows, H):
    """the stable partition and its offsets"""
    home = np_home(rec, wl, n_rows, H)
    order = np.argsort(home, kind="stable")
    off = np.zeros(H + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount(home, minlength=H))
    return rec[order], off


def records(wl, n, seed, one_key=False):
    """n canonical records over every table of the workload: random keys, values, versions, deletes and pad bytes"""
    rng = np.random.default_rng(seed)
    nt = len(hash_sizes(wl, 1000))
    rec = np.zeros(n, wire.LOG_REC)
    raw = rec.view(np.uint8).reshape(n, 64)
    raw[:] = rng.integers(0, 256, (n, 64), dtype=np.uint8)  # (pad bytes too: the route moves 64 bytes, whatever they are)
    rec["key"] = 77 if one_key else rng.integers(1, 1 << 44, n, dtype=np.uint64)
    rec["table"] = 0 if one_key else rng.integers(0, nt, n)
    return rec


def route_host(wl, n_rows, H, rec, fill=0xEE):
    rec = np.ascontiguousarray(rec)
    out = np.full(max(len(rec), 1) * 64 + 64, fill, np.uint8)  # (a guard record behind the output)
    off = np.full(H + 2, 0xEEEEEEEEEEEEEEEE, np.uint64)
    rc = _lib.load().dint_records_route_host(int(wl), n_rows, H, rec.ctypes.data if len(rec) else None, len(rec), out.ctypes.data,
                                             off.ctypes.data)
    return rc, out, off


def test_tile_constant_matches_the_library_and_the_header():
    assert _lib.load().dint_records_route_tile() == _lib.ROUTE_TILE
    src = open(os.path.join(ROOT, "dint_amd", "csrc", "state_route.h")).read()
    assert int(re.search(r"#define RR_TILE (\d+)u", src).group(1)) == _lib.ROUTE_TILE
    assert int(re.search(r"#define RR_MAX_SHARDS (\d+)u", src).group(1)) == _lib.ROUTE_MAX_SHARDS == 255
    hdr = open(os.path.join(ROOT, "include", "dint_abi.h")).read()
    assert int(re.search(r"#define DINT_FLAG_SHARD_REPLICA (0x[0-9a-f]+)u", hdr).group(1), 16) == _lib.FLAG_SHARD_REPLICA == 32


@pytest.mark.parametrize("wl,n_rows", SHAPES)
@pytest.mark.parametrize("H", HS)
def test_route_equals_a_stable_argsort_by_home(wl, n_rows, H):
    for n, one_key in ((0, False), (1, False), (1, True), (700, True), (2000, False)):
        rec = records(wl, n, seed=n + H, one_key=one_key)
        want, woff = np_route(rec, wl, n_rows, H)
        rc, out, off = route_host(wl, n_rows, H, rec)
        assert rc == n
        assert (off[:H + 1] == woff).all() and off[H + 1] == 0xEEEEEEEEEEEEEEEE
        assert out[:n * 64].tobytes() == want.tobytes()
        assert (out[n * 64:] == 0xEE).all()
        if one_key and n:
            assert (np.diff(woff.astype(np.int64)) > 0).sum() == 1  # one shard takes everything
            assert out[:n * 64].tobytes() == rec.tobytes()
        if n == 2000:
            assert len(np.unique(rec["table"])) == len(hash_sizes(wl, n_rows))  # all tables mixed
            if H == 1:
                assert out[:n * 64].tobytes() == rec.tobytes()  # one shard: a copy


def test_most_shards_are_empty_at_255_with_few_records():
    rec = records(W.TATP, 40, seed=9)
    rc, out, off = route_host(W.TATP, 300, 255, rec)
    assert rc == 40 and (np.diff(off[:256].astype(np.int64)) == 0).sum() >= 215
    assert out[:40 * 64].tobytes() == np_route(rec, W.TATP, 300, 255)[0].tobytes()


def test_a_routed_list_in_bucket_order_is_in_local_bucket_order_in_every_shard():
    """the order dint_state_diff writes (table, global bucket ascending) survives the route as (table, global bucket // H)"""
    wl, n_rows = W.TATP, 300
    rec = records(wl, 3000, seed=4)
    hs = hash_sizes(wl, n_rows)
    g = np.zeros(len(rec), np.int64)
    for t, h in enumerate(hs):
        m = rec["table"] == t
        g[m] = np_bucket(rec["key"][m], h).astype(np.int64)
    o = np.lexsort((g, rec["table"]))
    rec, g = rec[o], g[o]
    for H in (2, 3, 5):
        rc, out, off = route_host(wl, n_rows, H, rec)
        got = np.frombuffer(out[:len(rec) * 64].tobytes(), wire.LOG_REC)
        for h in range(H):
            piece = got[int(off[h]):int(off[h + 1])]
            lg = np.zeros(len(piece), np.int64)
            for t, hsz in enumerate(hs):
                m = piece["table"] == t
                gb = np_bucket(piece["key"][m], hsz).astype(np.int64)
                assert (gb % H == h).all()
                lg[m] = gb // H
            place = piece["table"].astype(np.int64) << 40 | lg
            assert (np.diff(place) >= 0).all()


def test_refusals_leave_the_output_as_it_was():
    L = _lib.load()
    rec = records(W.TATP, 100, seed=1)
    bad = rec.copy()
    bad["table"][61] = 5
    bad["table"][90] = 200
    for wl, n_rows, r in ((W.TATP, 300, bad), (W.SMALLBANK, 1000, records(W.TATP, 100, seed=2))):
        if wl == W.SMALLBANK:
            r["table"][:] = 1
            r["table"][17] = 2
        rc, out, off = route_host(wl, n_rows, 3, r)
        assert rc == EINVAL and (out == 0xEE).all() and (off == 0xEEEEEEEEEEEEEEEE).all()
        assert (b"record 61 " if wl == W.TATP else b"record 17 ") in L.dint_last_error()
    out = np.full(101 * 64, 0xEE, np.uint8)
    off = np.zeros(300, np.uint64)
    for H in (0, 256, 70000):
        assert L.dint_records_route_host(int(W.TATP), 300, H, rec.ctypes.data, 100, out.ctypes.data, off.ctypes.data) == EINVAL
    assert L.dint_records_route_host(int(W.TATP), 300, 2, rec.ctypes.data, 100, out.ctypes.data, None) == EINVAL
    assert L.dint_records_route_host(int(W.TATP), 300, 2, None, 100, out.ctypes.data, off.ctypes.data) == EINVAL
    assert L.dint_records_route_host(int(W.TATP), 300, 2, rec.ctypes.data, 100, None, off.ctypes.data) == EINVAL
    for wl in (W.FASST, W.TPL, W.LOG):
        assert L.dint_records_route_host(int(wl), 300, 2, rec.ctypes.data, 100, out.ctypes.data, off.ctypes.data) == ESTATE
    assert (out == 0xEE).all() and (off == 0).all()
    # overlapping ranges, either way round
    both = np.full(200 * 64, 0xEE, np.uint8)
    both[:100 * 64] = rec.view(np.uint8)
    before = both.copy()
    p = both.ctypes.data
    assert L.dint_records_route_host(int(W.TATP), 300, 2, p, 100, p + 64 * 99, off.ctypes.data) == EINVAL
    assert L.dint_records_route_host(int(W.TATP), 300, 2, p + 64, 99, p, off.ctypes.data) == EINVAL
    assert L.dint_records_route_host(int(W.TATP), 300, 2, p, 100, p, off.ctypes.data) == EINVAL
    assert (both == before).all() and (off == 0).all()
    assert L.dint_records_route_host(int(W.TATP), 300, 2, p, 100, p + 64 * 100, off.ctypes.data) == 100  # adjacent: fine
    # no records: every offset 0, nothing else touched
    off[:] = 7
    assert L.dint_records_route_host(int(W.TATP), 300, 4, None, 0, None, off.ctypes.data) == 0
    assert (off[:5] == 0).all() and (off[5:] == 7).all()


def test_records_at_an_odd_address():
    rec = records(W.STORE, 300, seed=3)
    raw = np.zeros(300 * 64 + 1, np.uint8)
    raw[1:] = rec.view(np.uint8)
    out = np.full(300 * 64 + 3, 0xEE, np.uint8)
    off = np.zeros(6, np.uint64)
    rc = _lib.load().dint_records_route_host(int(W.STORE), 1000, 5, raw.ctypes.data + 1, 300, out.ctypes.data + 3, off.ctypes.data)
    want, woff = np_route(rec, W.STORE, 1000, 5)
    assert rc == 300 and (off == woff).all() and out[3:].tobytes() == want.tobytes() and (out[:3] == 0xEE).all()
