"""The held locks' rule without a GPU (dint_amd/csrc/state_locks.h through dint_state_locks_image_host and
dint_state_unlock_check_host, include/dint_driver.h) against a numpy / Python form written from the format comment of
state_image.h and the table of include/dint_abi.h alone: it parses the image, follows the image-relative links and hashes with
the fasthash of tests/shard_double.py, and shares no code with the rule.  Every comparison is exact.

`python tests/test_state_locks_host.py FILE` writes the hand-built images below with the numpy form's lists, and the list-check
cases with the indices they must be refused at, into FILE for the stand-alone sanitizer program tests/native/state_locks_main.cc."""
import ctypes as C
import os
import struct
import subprocess
import sys

if __name__ == "__main__":  # (run as a script: pytest's conftest is not there to put the repository on the path)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import pytest

from dint_amd import _lib, wire
from shard_double import fasthash_key
from test_state_image_host import HDR_FMT
from test_state_stats_host import bucket, build_image, entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = wire.Workload
EINVAL, ESTATE = -1, -5
KEY_OWNER, KEY_ROW, WALK_CUT = 1, 2, 4
SAME_KEY = 4  # DINT_FLAG_LOCK_SAME_KEY
REC = np.dtype([("slot", "<u8"), ("a", "<u4"), ("b", "<u4"), ("key", "<u8"), ("cand_rows", "<u4"), ("table", "u1"), ("flags", "u1"), ("zero", "<u2")])
assert REC.itemsize == 32
STAT_KEYS = ("total", "held", "sum_a", "sum_b", "no_row", "walk_cut")


# ------------------------------------------------------------------------------------------------ the numpy / Python form
def np_held(workload, a, b):
    return a != 0 if workload == int(W.FASST) else (a != 0 or b != 0)


def np_image_locks(image_bytes):
    """(records, stats) of an image, from its bytes alone"""
    img = np.frombuffer(bytes(image_bytes), np.uint8)
    h = struct.unpack(HDR_FMT, img[:320].tobytes())
    workload, flags, n_tables, stride, src_count = h[2], h[3], h[4], h[5], h[8]
    recs, st = [], {"total": 0, "held": [0] * 5, "sum_a": 0, "sum_b": 0, "no_row": 0, "walk_cut": 0}
    for t in range(n_tables):
        size, n_b, n_ovf, _, off = h[13 + 5 * t:18 + 5 * t]
        d = img[off:off + 16 * n_b]
        ids = d.view("<u8").reshape(n_b, 2)[:, 0] if n_b else np.zeros(0, "<u8")
        if stride == 8:  # a lock table: {u64 global slot, u32 a, u32 b}
            ab = d.view("<u4").reshape(n_b, 4)[:, 2:] if n_b else np.zeros((0, 2), "<u4")
            for i in range(n_b):
                a, b = int(ab[i, 0]), int(ab[i, 1])
                if np_held(workload, a, b):
                    recs.append((int(ids[i]) // src_count, a, b, 0, 0, t, 0, 0))
            continue
        n_local = (size + src_count - 1) // src_count
        inl = img[off + 16 * n_b:off + 16 * n_b + n_b * stride].reshape(n_b, stride)
        ovf = img[off + 16 * n_b + n_b * stride:][:n_ovf * stride].reshape(n_ovf, stride)
        for i in range(n_b):
            gid = int(ids[i])
            for q in range(4):
                if workload == int(W.TATP):
                    a, b = int(inl[i, 60 + q]), 0
                else:
                    a, b = (int(x) for x in inl[i, 96 + 8 * q:104 + 8 * q].view("<u4"))
                if not np_held(workload, a, b):
                    continue
                keys, link, seen_inline, n = [], int(inl[i, 56:60].view("<u4")[0]), False, 0
                while link:  # (the hand-built chains end: no cut here)
                    assert n < 4096 and not (link == 1 and seen_inline)
                    seen_inline |= link == 1
                    e = inl[i] if link == 1 else ovf[link - 2]
                    keys += e[:32].view("<u8")[e[48:52] != 0].tolist()
                    link, n = int(e[52:56].view("<u4")[0]), n + 1
                want = q * size + gid
                cand = [k for k in keys if int(fasthash_key(np.array([k], "<u8"))[0] % np.uint64(4 * size)) == want]
                fl, key = (KEY_ROW if cand else 0), (cand[0] if cand else 0)
                if workload == int(W.TATP) and flags & SAME_KEY:
                    fl, key = KEY_OWNER, int(inl[i, 224 + 8 * q:232 + 8 * q].view("<u8")[0])
                st["no_row"] += not cand
                recs.append((q * n_local + gid // src_count, a, b, key, len(cand), t, fl, 0))
    for r in recs:
        st["total"] += 1
        st["held"][r[5]] += 1
        st["sum_a"] += r[1]
        st["sum_b"] += r[2]
    return np.array(recs, REC) if recs else np.zeros(0, REC), st


def host_locks(img, cap=None):
    """the host form: (return value, records, stats) or (rc, message)"""
    img = np.ascontiguousarray(img, np.uint8)
    L = _lib.load()
    s = _lib.LockStats()
    if cap is None:
        n = L.dint_state_locks_image_host(img.ctypes.data, img.nbytes, None, 0, C.byref(s))
        if n < 0:
            return n, L.dint_last_error().decode()
        assert n == 0
        cap = int(s.total)
    out = np.zeros(cap + 1, REC)
    out["zero"] = 0xABCD  # a guard behind the cap records
    n = L.dint_state_locks_image_host(img.ctypes.data, img.nbytes, out.ctypes.data, cap, C.byref(s))
    if n < 0:
        return n, L.dint_last_error().decode()
    assert out[cap]["zero"] == 0xABCD and not out[cap]["slot"]
    return n, out[:n], s.as_dict()


def key_for(size, lock_hash, nth=0, start=1):
    """the nth key >= start with fasthash64(key) % (4 * size) == lock_hash"""
    k = start
    while True:
        c = np.arange(k, k + 4096, dtype="<u8")
        hit = c[fasthash_key(c) % np.uint64(4 * size) == np.uint64(lock_hash)]
        if len(hit) > nth:
            return int(hit[nth])
        nth -= len(hit)
        k += 4096


# ------------------------------------------------------------------------------------------------ hand-built images
def lock_image(workload, n_slots, slots, src=(0, 1), dst=(0, 1)):
    """slots: [(global slot, a, b)] ascending -> the image of a lock table, laid out as state_image.h says"""
    body = b"".join(struct.pack("<QII", *s) for s in slots)
    rows = sum(1 for _, a, b in slots if a or b)
    tabs = [n_slots, len(slots), 0, rows, 320] + [0] * 20
    hdr = struct.pack(HDR_FMT, 0x31474D49544E4944, 1, int(workload), 0, 1, 8, 0, src[0], src[1], dst[0], dst[1], 320 + len(body), 0, *tabs)
    return np.frombuffer(hdr + body, np.uint8).copy()


def with_owners(img, owners):
    """a tatp image with DINT_FLAG_LOCK_SAME_KEY set; owners: {(table, bucket index in the image, q): key}"""
    img = img.copy()
    img[16:20] = np.frombuffer(struct.pack("<I", SAME_KEY), np.uint8)
    h = struct.unpack(HDR_FMT, img[:320].tobytes())
    for (t, i, q), key in owners.items():
        _, n_b, _, _, off = h[13 + 5 * t:18 + 5 * t]
        at = off + 16 * n_b + i * 256 + 224 + 8 * q
        img[at:at + 8] = np.frombuffer(struct.pack("<Q", key), np.uint8)
    return img


SZ = 7  # global buckets of every table of the kv cases: 28 lock slots a table


def cases():
    c = []
    k = lambda g, q, nth=0: key_for(SZ, q * SZ + g, nth)  # noqa: E731
    c.append(("tatp_nothing_held", build_image(W.TATP, [[bucket(1, [("I", entry([k(1, 0)]))])], [], [], [], []], global_size=SZ)))
    # bucket 2: unit q=0 with a row, q=1 without one, q=3 with two keys of the unit (one behind a hole, one in an overflow entry);
    # bucket 5: the inline entry in the middle of the chain, a key held twice (the first in chain order is in the overflow entry)
    dup = k(5, 2)
    t0 = [bucket(2, [("O", entry([k(2, 3), None, k(2, 2)])), ("I", entry([None, k(2, 0), k(2, 3, 1)], lockw=(1, 1, 0, 1)))]),
          bucket(5, [("O", entry([k(5, 1), dup])), ("I", entry([dup, k(5, 2, 1)], lockw=(0, 0, 7, 0))), ("O", entry([k(5, 0)]))])]
    t3 = [bucket(0, [], inline=entry(lockw=(0, 0, 0, 1))), bucket(6, [("I", entry([k(6, 1), k(6, 1, 1), k(6, 1, 2), k(6, 2)], lockw=(9, 1, 0, 0)))])]
    tatp = build_image(W.TATP, [t0, [], [], t3, []], global_size=SZ)
    c.append(("tatp_candidates", tatp))
    c.append(("tatp_owner_keys", with_owners(tatp, {(0, 0, 0): k(2, 0), (0, 0, 1): 12345, (0, 0, 3): k(2, 3, 1), (0, 1, 2): dup, (3, 1, 0): 77})))
    sb = lambda ks, cnt=None: entry(ks, stride=128, counters=cnt)  # noqa: E731
    c.append(("smallbank_two_tables", build_image(W.SMALLBANK, [
        [bucket(0, [("I", sb([k(0, 0), k(0, 3)], (1, 0, 0, 0, 0, 3, 2, 2)))]), bucket(4, [("O", sb([k(4, 3)])), ("I", sb([k(4, 0), k(4, 1)], (0, 0, 0, 0, 0, 0, 0, 1)))])],
        [bucket(2, [("I", sb([])), ("O", sb([k(2, 1), k(2, 1)]))]), bucket(3, [], inline=sb([], (0, 9, 0, 0, 0, 0, 0, 0)))]], global_size=SZ)))
    # a shard's own image: shard 1 of 3 of a table of 20 buckets holds the global buckets 1, 4, .. 19: local 0 .. 6
    ks = lambda g, q: key_for(20, q * 20 + g)  # noqa: E731
    c.append(("tatp_sharded", build_image(W.TATP, [[bucket(4, [("I", entry([ks(4, 2)], lockw=(0, 0, 1, 0)))]), bucket(19, [("I", entry([ks(19, 3)], lockw=(1, 0, 0, 1)))])],
                                                   [], [], [], []], src=(1, 3), dst=(1, 3), global_size=20)))
    c.append(("fasst_versions", lock_image(W.FASST, 10, [(0, 0, 5), (1, 1, 0), (2, 1, 9), (3, 0, 0), (9, 0, 1)])))
    c.append(("tpl_counters", lock_image(W.TPL, 10, [(0, 0, 0), (1, 1, 0), (2, 0, 3), (3, 2, 2)])))
    c.append(("fasst_sharded", lock_image(W.FASST, 1000, [(2, 1, 0), (5, 0, 7), (998, 1, 4)], src=(2, 3), dst=(2, 3))))
    c.append(("fasst_empty", lock_image(W.FASST, 10, [])))
    return c


CASES = cases()


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_host_form_equals_the_numpy_form(name):
    img = dict(CASES)[name]
    want, wst = np_image_locks(img)
    n, got, st = host_locks(img)
    assert n == len(want) and got.tobytes() == want.tobytes(), (got, want)
    assert {k: st[k] for k in STAT_KEYS} == wst
    # a cap below the total: the first records of the same order, the same statistics; counting alone writes nothing
    if len(want) > 1:
        n2, got2, st2 = host_locks(img, cap=len(want) - 1)
        assert n2 == len(want) - 1 and got2.tobytes() == want[:-1].tobytes() and st2 == st


def test_the_cases_are_what_they_claim():
    got = {n: np_image_locks(i) for n, i in CASES}
    assert got["tatp_nothing_held"][1]["total"] == 0
    r, st = got["tatp_candidates"]
    assert st["total"] == 7 and st["held"] == [4, 0, 0, 3, 0] and st["no_row"] == 3 and st["sum_a"] == 1 + 1 + 1 + 7 + 1 + 9 + 1
    assert r["slot"].tolist() == [0 * 7 + 2, 1 * 7 + 2, 3 * 7 + 2, 2 * 7 + 5, 3 * 7 + 0, 0 * 7 + 6, 1 * 7 + 6]  # bucket-major, then q
    assert r["cand_rows"].tolist() == [1, 0, 2, 3, 0, 0, 3] and r["flags"].tolist() == [2, 0, 2, 2, 0, 0, 2]
    assert r["key"][2] == key_for(SZ, 3 * SZ + 2) and r["key"][3] == key_for(SZ, 2 * SZ + 5)  # the first in CHAIN order: the overflow entry's
    o, _ = got["tatp_owner_keys"]
    assert (o["flags"] == KEY_OWNER).all() and o["key"].tolist()[1] == 12345 and o["key"].tolist()[4] == 0 and (o["cand_rows"] == r["cand_rows"]).all()
    s, st = got["smallbank_two_tables"]
    assert st["held"][:2] == [4, 1] and st["sum_a"] == 1 + 0 + 2 + 0 + 0 and st["sum_b"] == 0 + 3 + 2 + 1 + 9 and st["no_row"] == 2
    assert got["tatp_sharded"][0]["slot"].tolist() == [2 * 7 + 1, 0 * 7 + 6, 3 * 7 + 6]
    assert got["fasst_versions"][0]["slot"].tolist() == [1, 2] and got["fasst_versions"][0]["b"].tolist() == [0, 9]
    assert got["tpl_counters"][0]["slot"].tolist() == [1, 2, 3] and got["fasst_sharded"][0]["slot"].tolist() == [0, 332]


def test_image_refusals():
    img = dict(CASES)["tatp_candidates"]
    L = _lib.load()
    assert host_locks(img[:-16])[0] == EINVAL
    assert L.dint_state_locks_image_host(img.ctypes.data, img.nbytes, None, 3, None) == EINVAL
    assert L.dint_state_locks_image_host(img.ctypes.data, img.nbytes, None, 0, None) == 0  # (no statistics asked for)
    store = build_image(W.STORE, [[bucket(3, [("I", entry([7, 8]))])]])
    rc, msg = host_locks(store)
    assert rc == ESTATE and "no lock table" in msg


def test_struct_layout():
    assert C.sizeof(_lib.LockStats) == 128 and C.sizeof(_lib.UnlockStats) == 128 and C.sizeof(_lib.LockGeometry) == 56
    from dint_amd.engine import LOCK_REC
    assert LOCK_REC == REC


# ------------------------------------------------------------------------------------------------ the list check
def rec(slot, a=1, b=0, table=0, key=0, flags=0):
    return (slot, a, b, key, 0, table, flags, 0)


def np_first_bad(workload, geom, records):
    """the list check from the issue's list of refusals: geom = (shard_index, shard_count, [global sizes])"""
    idx, cnt, sizes = geom
    kv = workload in (int(W.TATP), int(W.SMALLBANK))
    prev = None
    for i, r in enumerate(records):
        t, slot = int(r["table"]), int(r["slot"])
        if t >= len(sizes):
            return i
        nl = (sizes[t] + cnt - 1) // cnt
        if slot >= (4 * nl if kv else nl):
            return i
        order = (t, slot % nl, slot // nl) if kv else (t, slot, 0)
        if kv and (slot % nl) * cnt + idx >= sizes[t]:
            return i
        if prev is not None and prev >= order:
            return i
        if r["a"] == 0 and (workload == int(W.FASST) or r["b"] == 0):
            return i
        prev = order
    return len(records)


def host_first_bad(workload, geom, records):
    g = _lib.LockGeometry(shard_index=geom[0], shard_count=geom[1], n_tables=len(geom[2]))
    for t, s in enumerate(geom[2]):
        g.size[t] = s
    r = np.ascontiguousarray(records)
    return int(_lib.load().dint_state_unlock_check_host(int(workload), C.byref(g), r.ctypes.data, len(r)))


TATP_G = (0, 1, [7, 7, 10, 10, 15])
LIST_CASES = [
    ("good_tatp", W.TATP, TATP_G, [rec(2), rec(9), rec(23), rec(5, table=0), rec(0, table=3), rec(39, table=3)], 6),
    ("empty", W.TATP, TATP_G, [], 0),
    ("bad_table", W.TATP, TATP_G, [rec(2), rec(0, table=5)], 1),
    ("bad_table_255", W.SMALLBANK, (0, 1, [7, 7]), [rec(0, table=255)], 0),
    ("sb_third_table", W.SMALLBANK, (0, 1, [7, 7]), [rec(0), rec(0, table=2)], 1),
    ("slot_past_4n", W.TATP, TATP_G, [rec(27), rec(28)], None),
    ("not_ascending_bucket", W.TATP, TATP_G, [rec(3), rec(2)], 1),
    ("q_descending_in_a_bucket", W.TATP, TATP_G, [rec(9), rec(2)], 1),
    ("q_ascending_in_a_bucket", W.TATP, TATP_G, [rec(2), rec(9), rec(16), rec(23)], 4),
    ("duplicate", W.TATP, TATP_G, [rec(2), rec(9), rec(9)], 2),
    ("table_descending", W.TATP, TATP_G, [rec(0, table=1), rec(1, table=0)], 1),
    ("holds_nothing", W.SMALLBANK, (0, 1, [7, 7]), [rec(0, a=0, b=2), rec(1, a=0, b=0)], 1),
    ("fasst_version_alone", W.FASST, (0, 1, [1000]), [rec(4), rec(5, a=0, b=3)], 1),
    ("tpl_shared_alone", W.TPL, (0, 1, [1000]), [rec(4), rec(5, a=0, b=3)], 2),
    ("lock_slot_range", W.FASST, (1, 3, [1000]), [rec(0), rec(333), rec(334)], 2),  # 334 local slots: 0 .. 333 (the last beyond the global range)
    ("lock_table_1", W.FASST, (0, 1, [1000]), [rec(0, table=1)], 0),
    ("sharded_bucket_beyond_the_table", W.TATP, (2, 3, [7, 7, 10, 10, 15]), [rec(1), rec(2)], 1),  # 3 local buckets; local 2 = global 8 >= 7
    ("sharded_q_of_3_local", W.TATP, (0, 3, [7, 7, 10, 10, 15]), [rec(2), rec(5), rec(11), rec(12)], 3),
    ("store_has_no_units", W.STORE, (0, 1, [288]), [rec(0)], 0),
]


@pytest.mark.parametrize("name", [c[0] for c in LIST_CASES])
def test_list_check_names_the_first_refused_record(name):
    _, wl, geom, recs, want = next(c for c in LIST_CASES if c[0] == name)
    r = np.array(recs, REC) if recs else np.zeros(0, REC)
    if wl == W.STORE:
        assert host_first_bad(wl, geom, r) == want
        return
    ref = np_first_bad(int(wl), geom, r)
    assert want is None or ref == want
    assert host_first_bad(wl, geom, r) == ref


def test_a_listing_and_its_subsequences_pass_the_check():
    """what the host form lists is a list; so is every sub-sequence of it, and no reversed one of two or more"""
    for name in ("tatp_candidates", "smallbank_two_tables", "tatp_sharded", "fasst_sharded", "tpl_counters"):
        img = dict(CASES)[name]
        h = struct.unpack(HDR_FMT, img[:320].tobytes())
        geom = (h[7], h[8], [h[13 + 5 * t] for t in range(h[4])])  # src_index, src_count, the global sizes
        _, r, _ = host_locks(img)
        for sub in (r, r[::2], r[1::3], r[:1]):
            assert host_first_bad(h[2], geom, sub) == len(sub)
        if len(r) > 1:
            assert host_first_bad(h[2], geom, r[::-1]) == 1


def write_fixtures(path):
    """u64 images, per image {u64 bytes, u64 records, the image padded to 8 bytes, the records, 10 u64 statistics}; then u64 lists,
    per list {u32 workload, struct dint_lock_geometry, u64 records, u64 the index it is refused at, the records}"""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(CASES)))
        for _, img in CASES:
            r, st = np_image_locks(img)
            f.write(struct.pack("<QQ", img.nbytes, len(r)))
            f.write(img.tobytes() + bytes(-img.nbytes % 8) + r.tobytes())
            f.write(struct.pack("<10Q", st["total"], *st["held"], st["sum_a"], st["sum_b"], st["no_row"], st["walk_cut"]))
        lists = [c for c in LIST_CASES if c[1] != W.STORE]
        f.write(struct.pack("<Q", len(lists)))
        for _, wl, geom, recs, _ in lists:
            r = np.array(recs, REC) if recs else np.zeros(0, REC)
            f.write(struct.pack("<I4I5Q", int(wl), geom[0], geom[1], len(geom[2]), 0, *(geom[2] + [0] * (5 - len(geom[2])))))
            f.write(struct.pack("<QQ", len(r), np_first_bad(int(wl), geom, r)) + r.tobytes())
    return len(CASES), len(lists)


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """tests/native/state_locks_main.cc with the host code of k_locks_state.hip and k_image.hip under AddressSanitizer and UBSan:
    images and lists in heap blocks of exactly their size, records at odd addresses.  Nothing of it is loaded into python"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe, fix = str(tmp_path / "state_locks_main"), str(tmp_path / "locks.bin")
    write_fixtures(fix)
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "native", "state_locks_main.cc"),
                           os.path.join(ROOT, "dint_amd", "csrc", "k_locks_state.hip"), os.path.join(ROOT, "dint_amd", "csrc", "k_image.hip"), "-o", exe])
    r = subprocess.run([exe, fix], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr


if __name__ == "__main__":
    print("%d images, %d lists" % write_fixtures(sys.argv[1]))
