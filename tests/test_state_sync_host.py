"""The state sync's rules on the host (dint_amd/csrc/state_sync.h through dint_state_row_hash_host / dint_state_digest_host /
dint_state_diff_host, include/dint_driver.h) against statements of the same rules that share no code with them: the CPU
oracle's fasthash64 for the row hash, a vectorised numpy fasthash64 (pinned against the oracle's below) for the digest, and
plain numpy set logic for the diff.  Plus the argument checks of the device calls (include/dint_abi.h dint_state_digest /
dint_state_diff / dint_state_repair) that need no device.

The GPU kernels of csrc/k_state.hip call the same state_sync.h functions; tests/test_gpu_state_sync.py holds them to the
numpy forms of this file end to end."""
import ctypes as C

import numpy as np
import pytest

from dint_amd import _lib, wire
from kvkeys import np_bucket  # noqa: F401  (other test modules import it from here)
from oracle import oracle as orc

EINVAL = -1
M64 = (1 << 64) - 1
SEED, FH_M, FH_K = 0xDEADBEEF, 0x880355F21E6D1965, 0x2127599BF4325C37


# ---- the reference forms (numpy; nothing of dint_amd below this line) ------------------------------------------------
def np_mix(h):
    h = h ^ (h >> np.uint64(23))
    h = h * np.uint64(FH_K)
    return h ^ (h >> np.uint64(47))


def np_fasthash64(buf: np.ndarray) -> np.ndarray:
    """fasthash64(row, L, 0xdeadbeef) of every row of an (n, L) uint8 array, L a multiple of 8 (lock_fasst/udp/utils.h:16-53)"""
    buf = np.ascontiguousarray(buf, np.uint8)
    n, length = buf.shape
    assert length % 8 == 0
    w = buf.view("<u8").reshape(n, length // 8)
    with np.errstate(over="ignore"):
        h = np.full(n, (SEED ^ (length * FH_M)) & M64, np.uint64)
        for k in range(length // 8):
            h = (h ^ np_mix(w[:, k])) * np.uint64(FH_M)
        return np_mix(h)


def canonical(table, keys, vers, vals) -> np.ndarray:
    """key (8, LE) | ver (4, LE) | table (1) | 0 0 0 | val"""
    keys, vers = np.ascontiguousarray(keys, "<u8"), np.ascontiguousarray(vers, "<u4")
    vals = np.ascontiguousarray(vals, np.uint8).reshape(len(keys), -1)
    out = np.zeros((len(keys), 16 + vals.shape[1]), np.uint8)
    out[:, 0:8] = keys.view(np.uint8).reshape(-1, 8)
    out[:, 8:12] = vers.view(np.uint8).reshape(-1, 4)
    out[:, 12] = table
    out[:, 16:] = vals
    return out


def np_digest(table, keys, vers, vals) -> dict:
    h = np_fasthash64(canonical(table, keys, vers, vals))
    return {"rows": len(h), "sum": int(h.sum(dtype=np.uint64)) if len(h) else 0,
            "xr": int(np.bitwise_xor.reduce(h)) if len(h) else 0}


def _visible(keys):
    """index of the first row of every key, in row order"""
    return np.sort(np.unique(keys, return_index=True)[1])


def np_diff(table, hash_size, a, b):
    """what must be done to b's visible rows to make them a's: (LOG_REC records in the contract's order, stats).  a, b =
    (keys, vers, vals) in dump order (bucket order is not needed; rows of one bucket keep their order)."""
    (ka, va, xa), (kb, vb, xb) = a, b
    xa, xb = np.asarray(xa).reshape(len(ka), -1), np.asarray(xb).reshape(len(kb), -1)
    ia, ib = _visible(ka), _visible(kb)
    ka, va, xa, kb, vb, xb = ka[ia], va[ia], xa[ia], kb[ib], vb[ib], xb[ib]
    in_b, in_a = np.isin(ka, kb), np.isin(kb, ka)
    ob = np.argsort(kb, kind="stable")
    at = ob[np.searchsorted(kb[ob], ka[in_b])]  # b's row of every key of a that b has
    val_diff, ver_diff = np.zeros(len(ka), bool), np.zeros(len(ka), bool)
    val_diff[in_b] = (xa[in_b] != xb[at]).any(axis=1)
    ver_diff[in_b] = va[in_b] != vb[at]
    ver_only = ver_diff & ~val_diff
    take_a = ~in_b | val_diff | ver_only
    ra = np.zeros(int(take_a.sum()), wire.LOG_REC)
    ra["key"], ra["ver"], ra["table"] = ka[take_a], va[take_a], table
    ra["val"][:, :xa.shape[1]] = xa[take_a]
    rb = np.zeros(int((~in_a).sum()), wire.LOG_REC)
    rb["key"], rb["is_del"], rb["table"] = kb[~in_a], 1, table
    rec = np.concatenate([ra, rb])
    side = np.concatenate([np.zeros(len(ra), np.int64), np.ones(len(rb), np.int64)])
    pos = np.concatenate([ia[take_a], ib[~in_a]])  # row order inside a side
    order = np.lexsort((pos, side, np_bucket(rec["key"], hash_size)))
    stats = {"total": len(rec), "only_a": int((~in_b).sum()), "only_b": int((~in_a).sum()), "val_differs": int(val_diff.sum()),
             "ver_only": int(ver_only.sum())}
    return rec[order], stats


# ---- the host exports -------------------------------------------------------------------------------------------------
def host_digest(table, keys, vers, vals, val_size) -> dict:
    L = _lib.load()
    keys, vers = np.ascontiguousarray(keys, "<u8"), np.ascontiguousarray(vers, "<u4")
    vals = np.ascontiguousarray(vals, np.uint8)
    d = _lib.TableDigest()
    assert L.dint_state_digest_host(table, keys.ctypes.data, vers.ctypes.data, vals.ctypes.data, val_size, len(keys), C.byref(d)) == 0
    return {"rows": d.rows, "sum": d.sum, "xr": d.xr}


def host_diff(table, hash_size, val_size, a, b, cap=None):
    L = _lib.load()
    arr = [np.ascontiguousarray(x, dt) for rows in (a, b) for x, dt in zip(rows, ("<u8", "<u4", np.uint8))]
    na, nb = len(arr[0]), len(arr[3])
    cap = na + nb if cap is None else cap
    rec = np.zeros(cap, wire.LOG_REC)
    st = _lib.DiffStats()
    n = L.dint_state_diff_host(table, hash_size, val_size, arr[0].ctypes.data, arr[1].ctypes.data, arr[2].ctypes.data, na,
                               arr[3].ctypes.data, arr[4].ctypes.data, arr[5].ctypes.data, nb, rec.ctypes.data, cap, C.byref(st))
    assert n >= 0
    return rec[:n], {k: getattr(st, k) for k, _ in st._fields_ if k != "reserved"}


def _random_rows(rng, n, val_size, key_bits=47):
    keys = rng.integers(0, 1 << key_bits, n, dtype=np.uint64)
    return keys, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype("<u4"), rng.integers(0, 256, (n, val_size), dtype=np.uint8)


# ---- tests ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [8, 24, 56, 64])
def test_numpy_fasthash64_is_the_oracles(length):
    rng = np.random.default_rng(length)
    buf = rng.integers(0, 256, (200, length), dtype=np.uint8)
    got = np_fasthash64(buf)
    assert [int(x) for x in got] == [orc.fasthash64(buf[i].tobytes()) for i in range(len(buf))]


@pytest.mark.parametrize("val_size", [40, 8])
def test_row_hash_is_fasthash64_of_the_canonical_bytes(val_size):
    L = _lib.load()
    rng = np.random.default_rng(val_size)
    keys, vers, vals = _random_rows(rng, 300, val_size, key_bits=64)
    tables = rng.integers(0, 5, 300)
    for i in range(300):
        can = canonical(int(tables[i]), keys[i:i + 1], vers[i:i + 1], vals[i:i + 1])[0].tobytes()
        assert len(can) == 16 + val_size
        got = L.dint_state_row_hash_host(int(keys[i]), int(vers[i]), int(tables[i]), vals[i].ctypes.data, val_size)
        assert got == orc.fasthash64(can)
    assert L.dint_state_row_hash_host(1, 2, 3, vals[0].ctypes.data, 16) == 0  # no such value size


@pytest.mark.parametrize("val_size", [40, 8])
def test_digest_equals_numpy_and_ignores_the_order_of_the_rows(val_size):
    rng = np.random.default_rng(100 + val_size)
    keys, vers, vals = _random_rows(rng, 5000, val_size)
    keys[17] = keys[4000]  # a duplicated key: two rows, both counted
    want = np_digest(3, keys, vers, vals)
    assert host_digest(3, keys, vers, vals, val_size) == want and want["rows"] == 5000
    p = rng.permutation(5000)
    assert host_digest(3, keys[p], vers[p], vals[p], val_size) == want
    assert host_digest(3, keys[:0], vers[:0], vals[:0], val_size) == {"rows": 0, "sum": 0, "xr": 0}
    # one bit of key, version, value or table: another digest
    seen = {(want["sum"], want["xr"])}
    for what in ("key", "ver", "val", "table"):
        for bit in (0, 5, 31):
            k2, v2, x2, t2 = keys.copy(), vers.copy(), vals.copy(), 3
            if what == "key":
                k2[123] ^= np.uint64(1 << bit)
            elif what == "ver":
                v2[123] ^= np.uint32(1 << bit)
            elif what == "val":
                x2[123, (bit // 8) % val_size] ^= np.uint8(1 << (bit % 8))
            else:
                t2 = 3 ^ (1 << (bit % 3))
            d = host_digest(t2, k2, v2, x2, val_size)
            assert d == np_digest(t2, k2, v2, x2) and d["rows"] == 5000
            assert (d["sum"], d["xr"]) not in seen, (what, bit)
            seen.add((d["sum"], d["xr"]))


@pytest.mark.parametrize("val_size,seed", [(40, 0), (40, 1), (8, 2)])
def test_diff_equals_numpy_set_logic_in_the_contracts_order(val_size, seed):
    rng = np.random.default_rng(seed)
    hash_size = 211  # few buckets: a dozen rows each, so the order inside a bucket is exercised
    keys, vers, vals = _random_rows(rng, 3000, val_size)
    a = [keys[:2400].copy(), vers[:2400].copy(), vals[:2400].copy()]
    pick = rng.permutation(3000)[:2500]  # b: most of a's rows in another order, plus 600 of its own
    b = [keys[pick].copy(), vers[pick].copy(), vals[pick].copy()]
    common = np.flatnonzero(pick < 2400)
    b[1][common[:300]] += 1                       # version only
    b[2][common[300:700], 3] ^= 0x10              # value (and for half of them the version too)
    b[1][common[300:500]] += 7
    a[0][5], a[0][9] = a[0][1000], a[0][1001]     # duplicated keys in a ...
    b[0][11] = b[0][2000]                          # ... and in b: the first row of a key is the visible one
    want, wst = np_diff(2, hash_size, a, b)
    got, gst = host_diff(2, hash_size, val_size, a, b)
    assert gst == wst and wst["total"] == len(want) == wst["only_a"] + wst["only_b"] + wst["val_differs"] + wst["ver_only"]
    assert min(wst["only_a"], wst["only_b"], wst["val_differs"], wst["ver_only"]) > 50
    assert got.tobytes() == want.tobytes()
    assert (got["pad"] == 0).all() and (got["val"][got["is_del"] != 0] == 0).all() and (got["ver"][got["is_del"] != 0] == 0).all()
    if val_size == 8:
        assert (got["val"][:, 8:] == 0).all()
    bk = np_bucket(got["key"], hash_size)
    assert (np.diff(bk.astype(np.int64)) >= 0).all()  # ascending bucket; inside a bucket a's rows before the b-only ones
    same = bk[1:] == bk[:-1]
    assert (got["is_del"][1:][same] >= got["is_del"][:-1][same]).all()
    # a smaller buffer takes a prefix and still says how many there are; equal sets have nothing to say
    part, pst = host_diff(2, hash_size, val_size, a, b, cap=100)
    assert pst == wst and part.tobytes() == want[:100].tobytes()
    none, nst = host_diff(2, hash_size, val_size, a, [x.copy() for x in a])
    assert len(none) == 0 and nst["total"] == 0


def test_device_calls_check_their_arguments_before_any_device_call():
    L = _lib.load()
    dg, df, rp = (_lib.TableDigest * 5)(), _lib.DiffStats(), _lib.RepairStats()
    fake = C.c_void_p(4096)  # never dereferenced: the checks below fail before an engine is looked at
    assert L.dint_state_digest(None, dg, 5, None) == EINVAL and b"null" in L.dint_last_error()
    assert L.dint_state_diff(None, None, None, 0, C.byref(df), None) == EINVAL
    assert L.dint_state_diff(fake, None, None, 0, None, None) == EINVAL
    assert L.dint_state_diff(None, fake, None, 0, None, None) == EINVAL
    assert L.dint_state_diff(fake, fake, None, 0, C.byref(df), None) == EINVAL and b"itself" in L.dint_last_error()
    assert L.dint_state_repair(None, None, 0, C.byref(rp), None) == EINVAL
    assert L.dint_state_repair(None, 4096, 10, None, None) == EINVAL
    assert L.dint_state_digest_host(0, None, None, None, 40, 5, C.byref(dg[0])) == EINVAL
    assert L.dint_state_digest_host(0, None, None, None, 40, 0, None) == EINVAL
    assert L.dint_state_diff_host(0, 0, 40, None, None, None, 0, None, None, None, 0, None, 0, None) == EINVAL  # hash_size 0
    assert L.dint_state_diff_host(0, 7, 40, None, None, None, 0, None, None, None, 0, None, 0, None) == 0
    assert C.sizeof(_lib.TableDigest) == 32 and C.sizeof(_lib.DiffStats) == 64 and C.sizeof(_lib.RepairStats) == 64
    assert _lib.ABI_VERSION == 5
    for name in ("dint_state_digest", "dint_state_diff", "dint_state_repair"):
        assert name in _lib.SYMBOLS
