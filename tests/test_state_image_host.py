"""The state image's rules without a GPU (dint_amd/csrc/state_image.h through dint_state_image_check_host, include/dint_driver.h;
dint_amd/recovery.py image_pieces), and the numpy reference forms the GPU tests (tests/test_gpu_state_image.py) hold the
re-shard to: they share no code with the feature -- fasthash in numpy (tests/shard_double.py) over dump_rows / read_locks."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import tracegen
from dint_amd import _lib, recovery, wire
from oracle import oracle as orc
from kvkeys import np_bucket  # noqa: F401  (the GPU tests import it from here)

W = wire.Workload
EINVAL = -1


# ------------------------------------------------------------------------------------------------ numpy reference forms
def np_select(dump, hash_size, j, H):
    """the rows of a bucket-ordered dump that live on shard j of H: a stable selection"""
    keys, vers, vals = dump
    m = (np_bucket(keys, hash_size) % np.uint64(H)).astype(np.int64) == j
    return keys[m], vers[m], vals[m]


def np_merge(dumps, hash_size):
    """the dumps of a complete sharded set as one dump in global bucket order (a bucket lives on one shard: stable)"""
    keys = np.concatenate([d[0] for d in dumps]); vers = np.concatenate([d[1] for d in dumps]); vals = np.concatenate([d[2] for d in dumps])
    o = np.argsort(np_bucket(keys, hash_size), kind="stable")
    return keys[o], vers[o], vals[o]


def np_reshard(dumps, hash_size, H):
    """expected dump_rows of every shard j of H from the dumps of a complete source set"""
    whole = np_merge(dumps, hash_size)
    return [np_select(whole, hash_size, j, H) for j in range(H)]


def np_locks_global(locks, hash_size):
    """read_locks of a complete set of G shards (index q * n_local + local) as the unsharded arrays (index q * hash_size + g)"""
    G = len(locks)
    A, B = np.zeros(4 * hash_size, "<u4"), np.zeros(4 * hash_size, "<u4")
    for i, (a, b) in enumerate(locks):
        nl = len(a) // 4
        g = np.arange(nl, dtype=np.int64) * G + i
        ok = g < hash_size
        for q in range(4):
            A[q * hash_size + g[ok]] = a[q * nl:(q + 1) * nl][ok]
            B[q * hash_size + g[ok]] = b[q * nl:(q + 1) * nl][ok]
    return A, B


def np_locks_shard(A, B, hash_size, j, H):
    """expected read_locks of shard j of H from the unsharded arrays"""
    nl = (hash_size + H - 1) // H
    a, b = np.zeros(4 * nl, "<u4"), np.zeros(4 * nl, "<u4")
    g = np.arange(nl, dtype=np.int64) * H + j
    ok = g < hash_size
    for q in range(4):
        a[q * nl:(q + 1) * nl][ok] = A[q * hash_size + g[ok]]
        b[q * nl:(q + 1) * nl][ok] = B[q * hash_size + g[ok]]
    return a, b


def same_dump(x, y):
    return all(p.tobytes() == q.tobytes() for p, q in zip(x, y))


# ------------------------------------------------------------------------------------------------ image_pieces
@pytest.mark.parametrize("G,H", [(1, 8), (8, 1), (2, 3), (2, 4), (4, 2), (3, 3)])
def test_image_pieces_is_the_gcd_rule(G, H):
    brute = sorted({(g % G, g % H) for g in range(G * H * 3)})  # every residue pair some global bucket has
    got = recovery.image_pieces(G, H)
    assert got == brute
    d = math.gcd(G, H)
    assert got == [(i, j) for i in range(G) for j in range(H) if i % d == j % d] and len(got) == G * H // d


# ------------------------------------------------------------------------------------------------ hand-built images
STRIDE = 256
HDR_FMT = "<Q10IQQ" + "5Q" * 5 + "56x"
assert struct.calcsize(HDR_FMT) == 320


def _entry(valid=(1, 0, 0, 0), nxt=0, head=0, key0=7):
    e = np.zeros(STRIDE, np.uint8)
    e[0:8] = np.frombuffer(struct.pack("<Q", key0), np.uint8)
    e[48:52] = valid
    e[52:60] = np.frombuffer(struct.pack("<II", nxt, head), np.uint8)
    return e


def _image(buckets, global_size=100, src=(0, 1), dst=(0, 1)):
    """buckets: [(id, inline entry, [overflow entries])] -> a store image (one table of 256-byte entries)"""
    n_b = len(buckets)
    ovf = [o for _, _, os_ in buckets for o in os_]
    rows = sum(int((np.asarray(e[48:52]) != 0).sum()) for _, e, os_ in buckets for e in [e] + list(os_))
    off = 320
    body = bytearray()
    first = 0
    for gid, _, os_ in buckets:
        body += struct.pack("<QII", gid, first, len(os_))
        first += len(os_)
    for _, e, _ in buckets:
        body += e.tobytes()
    for o in ovf:
        body += o.tobytes()
    total = off + len(body)
    tabs = [global_size, n_b, len(ovf), rows, off] + [0] * 20
    hdr = struct.pack(HDR_FMT, 0x31474D49544E4944, 1, int(W.STORE), 0, 1, STRIDE, 40, src[0], src[1], dst[0], dst[1], total, 0, *tabs)
    return np.frombuffer(hdr + bytes(body), np.uint8).copy()


def _check(img, nbytes=None):
    L = _lib.load()
    rc = L.dint_state_image_check_host(img.ctypes.data, img.nbytes if nbytes is None else nbytes)
    return rc, L.dint_last_error().decode()


def _chain3():
    """one bucket: overflow 0 -> inline -> overflow 1"""
    return [(3, _entry(nxt=3, head=2), [_entry(nxt=1, key0=8), _entry(nxt=0, key0=9)])]


def test_check_accepts_well_formed_images():
    assert _check(_image([(3, _entry(nxt=0, head=1), [])]))[0] == 0
    assert _check(_image([(3, _entry(valid=(0, 0, 0, 0)), [])]))[0] == 0  # an empty bucket that carries lock bytes only
    assert _check(_image(_chain3()))[0] == 0
    assert _check(_image([], dst=(1, 2)))[0] == 0  # an empty piece
    two = [(4, _entry(nxt=0, head=2), [_entry(nxt=1)]), (10, _entry(nxt=3, head=1), [_entry(nxt=0)])]
    assert _check(_image(two, dst=(0, 2)))[0] == 0


def _set_link(img, n_b, where, field, value):
    """where = ("inl", b) or ("ovf", x); field = "next" / "head" """
    n_ovf_at = 320 + 16 * n_b + n_b * STRIDE
    at = 320 + 16 * n_b + where[1] * STRIDE if where[0] == "inl" else n_ovf_at + where[1] * STRIDE
    img[at + (52 if field == "next" else 56):][:4] = np.frombuffer(struct.pack("<I", value), np.uint8)
    return img


def _orphans():
    """a table of no buckets and one overflow entry: the sizes add up, but the entry belongs to no bucket's run"""
    img = _image([])
    img = np.concatenate([img, _entry(nxt=0, key0=9)])
    img[64 + 16:64 + 24] = np.frombuffer(struct.pack("<Q", 1), np.uint8)           # table 0: n_overflow = 1
    img[48:56] = np.frombuffer(struct.pack("<Q", img.nbytes), np.uint8)            # header.bytes
    return img


@pytest.mark.parametrize("case", ["truncated", "order", "range", "home", "beyond", "other_run", "skip", "revisit", "orphans"])
def test_check_refuses_one_malformation(case):
    two = [(4, _entry(nxt=0, head=2), [_entry(nxt=1)]), (10, _entry(nxt=3, head=1), [_entry(nxt=0)])]
    nbytes, what = None, None
    if case == "truncated":
        img, nbytes, what = _image(_chain3()), _image(_chain3()).nbytes - 16, "bytes"
    elif case == "order":
        img, what = _image([(10, two[0][1], two[0][2]), (4, two[1][1], two[1][2])], dst=(0, 2)), "ascending"
    elif case == "range":
        img, what = _image([(4, two[0][1], two[0][2]), (100, two[1][1], two[1][2])], dst=(0, 2)), "range"
    elif case == "home":
        img, what = _image([(4, two[0][1], two[0][2]), (11, two[1][1], two[1][2])], dst=(0, 2)), "home"
    elif case == "beyond":
        img, what = _set_link(_image(_chain3()), 1, ("ovf", 1), "next", 4), "beyond"  # entry 2 of 2: outside the image as well
    elif case == "other_run":
        img, what = _set_link(_image(two, dst=(0, 2)), 2, ("inl", 0), "head", 3), "beyond"  # bucket 4's head into bucket 10's run
    elif case == "orphans":
        img, what = _orphans(), "bytes"
    elif case == "skip":
        img, what = _set_link(_image(_chain3()), 1, ("inl", 0), "head", 3), "skips or revisits"  # straight to overflow entry 1
    else:
        img, what = _set_link(_image(_chain3()), 1, ("ovf", 1), "next", 2), "skips or revisits"  # back to overflow entry 0
    rc, msg = _check(img, nbytes)
    assert rc == EINVAL and what in msg, (rc, msg)


def test_check_refuses_what_is_no_image():
    img = _image(_chain3())
    assert _check(img, 100)[0] == EINVAL
    bad = img.copy(); bad[0] ^= 1
    assert _check(bad)[0] == EINVAL
    assert _lib.load().dint_state_image_check_host(None, 4096) == EINVAL
    inl = _image([(3, _entry(valid=(1, 0, 0, 0), nxt=0, head=0), [])])  # valid slots in an entry no chain reaches
    rc, msg = _check(inl)
    assert rc == EINVAL and "outside its chain" in msg


# ------------------------------------------------------------------------------------------------ the reference is self-consistent
def test_numpy_reshard_round_trip_on_an_oracle_dump():
    o = orc.TatpOracle(300, log_entries=1 << 16)
    existing = [o.dump(t)[0] for t in range(5)]
    o.replay(tracegen.tatp_random(6000, existing, seed=11, n_sub_touch=40))
    for t in range(5):
        hs = o.hash_size(t)
        d = o.dump(t)
        assert len(d[0]) > 0 and (np.diff(np_bucket(d[0], hs).astype(np.int64)) >= 0).all()  # bucket order
        three = np_reshard([d], hs, 3)
        assert sum(len(x[0]) for x in three) == len(d[0])
        for j, x in enumerate(three):
            assert ((np_bucket(x[0], hs) % np.uint64(3)) == j).all()
        assert same_dump(np_reshard(three, hs, 1)[0], d)
    A = np.arange(4 * 10, dtype="<u4") + 1
    parts = [np_locks_shard(A, A * 2, 10, j, 3) for j in range(3)]
    assert len(parts[0][0]) == 16 and same_dump(np_locks_global(parts, 10), (A, A * 2))
