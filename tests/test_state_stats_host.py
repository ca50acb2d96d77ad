"""The table report's rule without a GPU (dint_amd/csrc/state_stats.h through dint_state_stats_image_host, include/dint_driver.h)
against a numpy / Python form written from the format comment of state_image.h alone -- it parses the image's header,
directory, inline and overflow sections and follows the image-relative links, and shares no code with the rule -- and the
policy on top of the report (dint_amd/recovery.py hash_sizes / advise_n_rows / rehash_advice).  Every comparison is exact.

`python tests/test_state_stats_host.py FILE` writes the hand-built images below with the numpy form's reports into FILE, for the
stand-alone sanitizer program tests/native/state_stats_main.cc."""
import ctypes as C
import os
import struct
import sys
from fractions import Fraction

if __name__ == "__main__":  # (run as a script: pytest's conftest is not there to put the repository on the path)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import pytest

from dint_amd import _lib, recovery, wire
from test_state_image_host import HDR_FMT, _entry, _image

W = wire.Workload
EINVAL, ESTATE = -1, -5
NO_BUCKET = (1 << 64) - 1
DUP_MAX_CHAIN = 64  # state_stats.h ST_DUP_MAX_CHAIN
SHAPE = {W.STORE: (1, 256, 40), W.TATP: (5, 256, 40), W.SMALLBANK: (2, 128, 8)}  # tables, stride, value size
SCALARS = ("buckets", "buckets_empty", "rows", "entries", "overflow_entries", "holes", "inline_first", "inline_unlinked", "hit_entries",
           "shadowed_rows", "buckets_unchecked", "longest_chain", "longest_chain_bucket", "most_rows", "locks_held", "pool_cap", "pool_top")


# ------------------------------------------------------------------------------------------------ the numpy / Python form
def np_image_stats(image_bytes):
    """the report of every table of a kv image, from the bytes alone: list of dicts with every field of dint_table_stats"""
    img = np.frombuffer(bytes(image_bytes), np.uint8)
    h = struct.unpack(HDR_FMT, img[:320].tobytes())
    workload, n_tables, stride = h[2], h[4], h[5]
    out = []
    for t in range(n_tables):
        _, n_b, n_ovf, _, off = h[13 + 5 * t:18 + 5 * t]
        ids = img[off:off + 16 * n_b].view("<u8").reshape(n_b, 2)[:, 0] if n_b else np.zeros(0, "<u8")
        inl = img[off + 16 * n_b:off + 16 * n_b + n_b * stride].reshape(n_b, stride)
        ovf = img[off + 16 * n_b + n_b * stride:][:n_ovf * stride].reshape(n_ovf, stride)
        r = {k: 0 for k in SCALARS}
        r["longest_chain_bucket"] = NO_BUCKET
        r["chain_hist"], r["rows_hist"] = [0] * 17, [0] * 33
        r["buckets"] = n_b
        for b in range(n_b):
            link = int(inl[b, 56:60].view("<u4")[0])  # head
            chain, seen_inline = [], False
            while link:
                assert len(chain) < 4096
                if link == 1:
                    assert not seen_inline
                    seen_inline = True
                    e = inl[b]
                else:
                    e = ovf[link - 2]
                chain.append((link, e))
                link = int(e[52:56].view("<u4")[0])
            keys, hit = [], 0
            for pos, (_, e) in enumerate(chain):
                valid = e[48:52] != 0
                keys += e[:32].view("<u8")[valid].tolist()
                hit += (pos + 1) * int(valid.sum())
            rows, entries = len(keys), len(chain)
            r["rows"] += rows
            r["entries"] += entries
            r["overflow_entries"] += sum(1 for link, _ in chain if link != 1)
            r["buckets_empty"] += rows == 0
            r["inline_first"] += bool(chain) and chain[0][0] == 1
            r["inline_unlinked"] += bool(chain) and not seen_inline
            r["hit_entries"] += hit
            if entries > DUP_MAX_CHAIN and rows > 1:
                r["buckets_unchecked"] += 1
            else:
                r["shadowed_rows"] += rows - len(np.unique(np.array(keys, "<u8")))
            if entries > r["longest_chain"]:  # (ids ascend: the first bucket that attains it is the lowest)
                r["longest_chain"], r["longest_chain_bucket"] = entries, int(ids[b])
            r["most_rows"] = max(r["most_rows"], rows)
            r["chain_hist"][min(entries, 16)] += 1
            r["rows_hist"][min(rows, 32)] += 1
            if workload == int(W.TATP):
                r["locks_held"] += int((inl[b, 60:64] != 0).sum())
            elif workload == int(W.SMALLBANK):
                r["locks_held"] += int((inl[b, 96:128].view("<u4").reshape(4, 2) != 0).any(axis=1).sum())
        r["holes"] = 4 * r["entries"] - r["rows"]
        if r["rows"] == 0:
            r["longest_chain_bucket"] = NO_BUCKET
        out.append(r)
    return out


def assert_identities(r):
    """what every report satisfies, whatever made it (the issue's list)"""
    assert sum(r["chain_hist"]) == sum(r["rows_hist"]) == r["buckets"]
    assert r["rows_hist"][0] == r["buckets_empty"]
    if r["longest_chain"] < 16:
        assert sum(k * c for k, c in enumerate(r["chain_hist"])) == r["entries"]
    # entries - overflow_entries = the buckets whose chain contains the inline entry = the non-empty chains but the unlinked ones
    assert r["entries"] - r["overflow_entries"] == r["buckets"] - r["chain_hist"][0] - r["inline_unlinked"]
    assert r["holes"] == 4 * r["entries"] - r["rows"]
    assert (r["longest_chain_bucket"] == NO_BUCKET) == (r["rows"] == 0)


def host_stats(img, cap=5):
    img = np.ascontiguousarray(img, np.uint8)
    out = (_lib.TableStats * 5)()
    L = _lib.load()
    rc = L.dint_state_stats_image_host(img.ctypes.data, img.nbytes, out, cap)
    if rc < 0:
        return rc, L.dint_last_error().decode()
    return rc, [out[t].as_dict() for t in range(rc)]


# ------------------------------------------------------------------------------------------------ hand-built images
def entry(keys=(), stride=256, lockw=(0, 0, 0, 0), counters=None):
    """keys: up to four, None = a hole; links are set by build_image"""
    e = np.zeros(stride, np.uint8)
    for i, k in enumerate(keys):
        if k is not None:
            e[8 * i:8 * i + 8] = np.frombuffer(struct.pack("<Q", k), np.uint8)
            e[32 + 4 * i:36 + 4 * i] = np.frombuffer(struct.pack("<I", i + 1), np.uint8)
            e[48 + i] = 1
    e[60:64] = lockw
    if counters is not None:
        e[96:128] = np.frombuffer(struct.pack("<8I", *counters), np.uint8)
    return e


def bucket(gid, chain, inline=None):
    """chain: entries in chain order, ("I", entry) for the inline one, ("O", entry) for an overflow entry.  inline = the inline
    entry of a bucket whose chain does not contain it (no valid slot: an image never holds one there)"""
    return gid, chain, inline


def build_image(workload, tables, src=(0, 1), dst=(0, 1), global_size=1 << 20):
    """tables: per table a list of buckets (ascending ids) -> image bytes, laid out as state_image.h says"""
    n_tables, stride, val_size = SHAPE[workload]
    assert len(tables) == n_tables
    body, tabs, off = bytearray(), [], 320
    for buckets in tables:
        d, inl, ovf, rows = bytearray(), bytearray(), bytearray(), 0
        for gid, chain, unlinked in buckets:
            first, m, links = len(ovf) // stride, 0, []
            for kind, _ in chain:
                links.append(1 if kind == "I" else first + m + 2)
                m += kind == "O"
            ie = (unlinked if unlinked is not None else entry(stride=stride)).copy()
            for p, (kind, e) in enumerate(chain):
                e = e.copy()
                e[52:56] = np.frombuffer(struct.pack("<I", links[p + 1] if p + 1 < len(chain) else 0), np.uint8)
                rows += int((e[48:52] != 0).sum())
                if kind == "I":
                    ie = e
                else:
                    ovf += e.tobytes()
            ie[56:60] = np.frombuffer(struct.pack("<I", links[0] if links else 0), np.uint8)
            d += struct.pack("<QII", gid, first, m)
            inl += ie.tobytes()
        tabs += [global_size, len(buckets), len(ovf) // stride, rows, off]
        body += d + inl + ovf
        off = 320 + len(body)
    tabs += [0] * (25 - len(tabs))
    hdr = struct.pack(HDR_FMT, 0x31474D49544E4944, 1, int(workload), 0, n_tables, stride, val_size, src[0], src[1], dst[0], dst[1], off, 0, *tabs)
    return np.frombuffer(hdr + bytes(body), np.uint8).copy()


def _k(base, n):
    return [base + i for i in range(n)]


def _full_chain(n_entries, key0, inline_at=0, rows=None):
    """a chain of n_entries entries with `rows` valid slots (default: all), keys key0 .., the inline entry at position inline_at"""
    rows = 4 * n_entries if rows is None else rows
    chain = []
    for p in range(n_entries):
        ks = [key0 + 4 * p + i if 4 * p + i < rows else None for i in range(4)]
        chain.append(("I" if p == inline_at else "O", entry(ks)))
    return chain


def cases():
    """(name, image) of every shape the issue lists"""
    c = []
    c.append(("empty_table", build_image(W.STORE, [[]])))
    c.append(("empty_buckets", build_image(W.STORE, [[bucket(0, []), bucket(1, [])]])))
    c.append(("one_bucket", build_image(W.STORE, [[bucket(3, [("I", entry([7, 8]))])]])))
    c.append(("inline_positions", build_image(W.STORE, [[
        bucket(2, [("I", entry(_k(10, 4))), ("O", entry(_k(20, 4))), ("O", entry(_k(30, 2)))]),                   # first
        bucket(5, [("O", entry(_k(40, 4))), ("I", entry(_k(50, 4))), ("O", entry(_k(60, 3)))]),                   # in the middle
        bucket(9, [("O", entry(_k(70, 1))), ("O", entry(_k(80, 4))), ("I", entry(_k(90, 4)))])]])))               # last
    c.append(("inline_unlinked", build_image(W.STORE, [[
        bucket(4, [("O", entry(_k(10, 3))), ("O", entry(_k(20, 4)))], inline=entry()), bucket(6, [("I", entry([1]))])]])))
    c.append(("all_holes_linked", build_image(W.STORE, [[
        bucket(1, [("O", entry([None, 5])), ("I", entry()), ("O", entry([None, None, 6]))]), bucket(2, [("I", entry())])]])))
    c.append(("dup_in_one_entry", build_image(W.STORE, [[bucket(7, [("I", entry([11, 12, 11, 11]))])]])))
    c.append(("dup_across_entries", build_image(W.STORE, [[
        bucket(7, [("O", entry([11, 12])), ("I", entry([13, 11, None, 12])), ("O", entry([11]))])]])))
    for n in (15, 16, 17):
        c.append((f"chain_{n}", build_image(W.STORE, [[bucket(0, _full_chain(n, 1000, inline_at=n - 1)), bucket(1, _full_chain(2, 5000))]])))
    for rows in (31, 32, 33):
        c.append((f"rows_{rows}", build_image(W.STORE, [[bucket(8, _full_chain(9, 2000, inline_at=3, rows=rows))]])))
    for n in (64, 65):
        ch = _full_chain(n, 3000, inline_at=1)
        ch[n - 1] = ("O", entry([3000 + 4 * (n - 1), 3002]))  # key 3002 sits in the first entry as well
        c.append((f"chain_{n}_dup", build_image(W.STORE, [[bucket(5, ch), bucket(6, [("I", entry([1, 1]))])]])))
    c.append(("longest_tie", build_image(W.STORE, [[
        bucket(3, _full_chain(2, 100)), bucket(11, _full_chain(3, 200)), bucket(12, _full_chain(3, 300, inline_at=2)), bucket(20, _full_chain(1, 400))]])))
    sb = lambda ks, cnt=None: entry(ks, stride=128, counters=cnt)  # noqa: E731
    c.append(("smallbank_two_tables", build_image(W.SMALLBANK, [
        [bucket(0, [("I", sb([1, 2], (1, 0, 0, 0, 0, 3, 2, 2)))]), bucket(4, [("O", sb([5])), ("I", sb([6, 7, 8, 9], (0, 0, 0, 0, 0, 0, 0, 1)))])],
        [bucket(2, [("I", sb([])), ("O", sb([3, 3]))]), bucket(3, [], inline=sb([], (0, 9, 0, 0, 0, 0, 0, 0)))]])))
    c.append(("sharded_ids", build_image(W.STORE, [[
        bucket(5, _full_chain(2, 10)), bucket(17, _full_chain(4, 50, inline_at=1)), bucket(29, _full_chain(4, 90))]], src=(1, 4), dst=(2, 3))))
    tt = [[bucket(1, [("I", entry([7], lockw=(1, 0, 0, 2)))]), bucket(2, [], inline=entry(lockw=(0, 1, 0, 0)))],
          [bucket(0, [("I", entry([7, 9]))])], [], [bucket(6, [("O", entry([4], lockw=(9, 9, 9, 9))), ("I", entry([5], lockw=(0, 0, 3, 0)))])], []]
    c.append(("tatp_lock_bytes", build_image(W.TATP, tt)))
    return c


CASES = cases()


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_host_form_equals_the_numpy_form(name):
    img = dict(CASES)[name]
    want = np_image_stats(img)
    rc, got = host_stats(img)
    assert rc == len(want), got
    for t, (g, w) in enumerate(zip(got, want)):
        assert g == w, (t, {k: (g[k], w[k]) for k in w if g[k] != w[k]})
        assert_identities(g)
        assert g["pool_cap"] == 0 and g["pool_top"] == 0


def test_the_cases_are_what_they_claim():
    """the numpy form's own numbers on the hand-built shapes: a case that does not reach its edge is void"""
    st = {n: np_image_stats(i) for n, i in CASES}
    assert st["empty_table"][0]["buckets"] == 0 and st["empty_table"][0]["longest_chain_bucket"] == NO_BUCKET
    assert st["empty_buckets"][0]["buckets_empty"] == 2 and st["empty_buckets"][0]["longest_chain_bucket"] == NO_BUCKET
    ip = st["inline_positions"][0]
    assert ip["inline_first"] == 1 and ip["entries"] == 9 and ip["overflow_entries"] == 6 and ip["rows"] == 30 and ip["holes"] == 6
    assert ip["hit_entries"] == (4 + 8 + 6) + (4 + 8 + 9) + (1 + 8 + 12)
    assert st["inline_unlinked"][0]["inline_unlinked"] == 1 and st["inline_unlinked"][0]["inline_first"] == 1
    ah = st["all_holes_linked"][0]
    assert ah["entries"] == 4 and ah["rows"] == 2 and ah["holes"] == 14 and ah["buckets_empty"] == 1 and ah["chain_hist"][1] == 1
    assert st["dup_in_one_entry"][0]["shadowed_rows"] == 2 and st["dup_across_entries"][0]["shadowed_rows"] == 3
    for n in (15, 16, 17):
        r = st[f"chain_{n}"][0]
        assert r["longest_chain"] == n and r["chain_hist"][min(n, 16)] == 1 and r["longest_chain_bucket"] == 0
    for rows in (31, 32, 33):
        r = st[f"rows_{rows}"][0]
        assert r["most_rows"] == rows and r["rows_hist"][min(rows, 32)] == 1
    a, b = st["chain_64_dup"][0], st["chain_65_dup"][0]
    assert a["buckets_unchecked"] == 0 and a["shadowed_rows"] == 2 and b["buckets_unchecked"] == 1 and b["shadowed_rows"] == 1  # (bucket 6's, not the long one's)
    assert st["longest_tie"][0]["longest_chain"] == 3 and st["longest_tie"][0]["longest_chain_bucket"] == 11
    assert [r["locks_held"] for r in st["smallbank_two_tables"]] == [4, 1] and st["smallbank_two_tables"][1]["shadowed_rows"] == 1
    assert st["sharded_ids"][0]["longest_chain_bucket"] == 17
    assert [r["locks_held"] for r in st["tatp_lock_bytes"]] == [3, 0, 0, 1, 0]


def test_refusals():
    img = dict(CASES)["inline_positions"]
    rc, msg = host_stats(img, cap=0)
    assert rc == EINVAL and "room for" in msg
    rc, msg = host_stats(dict(CASES)["tatp_lock_bytes"], cap=4)
    assert rc == EINVAL
    # one of test_state_image_host.py's malformations: a chain that goes back to an entry it has visited -- refused, not walked
    bad = _image([(3, _entry(nxt=3, head=2), [_entry(nxt=1, key0=8), _entry(nxt=0, key0=9)])])
    assert host_stats(bad)[0] == 1
    bad[320 + 16 + 256 + 256 + 52:][:4] = np.frombuffer(struct.pack("<I", 2), np.uint8)  # overflow entry 1: next = overflow entry 0
    rc, msg = host_stats(bad)
    assert rc == EINVAL and "skips or revisits" in msg
    rc, _ = host_stats(img[:-16])
    assert rc == EINVAL
    L = _lib.load()
    assert L.dint_state_stats_image_host(img.ctypes.data, img.nbytes, None, 5) == EINVAL
    # the image of a lock table passes the image's check and has no chains to report
    lock = struct.pack(HDR_FMT, 0x31474D49544E4944, 1, int(W.FASST), 0, 1, 8, 0, 0, 1, 0, 1, 320 + 16, 0, *([100, 1, 0, 1, 320] + [0] * 20))
    lock = np.frombuffer(lock + struct.pack("<QII", 5, 1, 0), np.uint8).copy()
    assert L.dint_state_image_check_host(lock.ctypes.data, lock.nbytes) == 0
    assert host_stats(lock)[0] == ESTATE


def test_struct_layout():
    assert C.sizeof(_lib.TableStats) == 640 and _lib.TableStats.chain_hist.offset == 17 * 8 and _lib.TableStats.rows_hist.offset == 34 * 8


# ------------------------------------------------------------------------------------------------ the advice
WL_ROWS = {W.STORE: [[0], [1], [2880], [12_345]], W.TATP: [[0] * 5, [2000, 2000, 5000, 5000, 7400], [10, 10, 10, 10, 9_000], [700, 0, 0, 0, 0]],
           W.SMALLBANK: [[0, 0], [5000, 5000], [1, 7_777]]}


@pytest.mark.parametrize("wl", [W.STORE, W.TATP, W.SMALLBANK])
def test_bucket_counts_and_advised_n_rows_against_a_brute_force_search(wl):
    # dint_kv_create's formulas, restated with the reference's own fractions: rows per subscriber x 3/2 / 4 slots
    per_sub = {W.STORE: [12], W.TATP: [1, 1, Fraction(5, 2), Fraction(5, 2), Fraction(15, 4)], W.SMALLBANK: [1, 1]}[wl]
    for n in (1, 2, 3, 7, 64, 1000, 2000, 99_999):
        got = recovery.hash_sizes(wl, n)
        assert len(got) == SHAPE[wl][0]
        for h, f in zip(got, per_sub):
            assert abs(h - n * f * Fraction(3, 8)) < 1 or h == 1, (n, h)
    assert recovery.hash_sizes(W.STORE, 64) == [288] and recovery.hash_sizes(W.TATP, 2000) == [750, 750, 1875, 1875, 2812]
    assert recovery.hash_sizes(W.SMALLBANK, 2000) == [750, 750] and recovery.hash_sizes(W.STORE, 16) == [72]
    for rows in WL_ROWS[wl]:
        for rpb in (Fraction(8, 3), Fraction(2), Fraction(4)):
            def fits(n):
                return all(h * rpb >= r for h, r in zip(recovery.hash_sizes(wl, n), rows))
            brute = next(n for n in range(1, 50_000) if fits(n))
            assert recovery.advise_n_rows(wl, rows, float(rpb)) == brute, (rows, rpb)


class _FakeEngine:
    """an engine as rehash_advice sees it: a workload, bucket counts and a report"""

    def __init__(self, wl, n_rows, reports):
        self.workload, self._hs, self._rep = wl, recovery.hash_sizes(wl, n_rows), reports

    def hash_size(self, t):
        return self._hs[t]

    def state_stats(self):
        return [dict(r) for r in self._rep]


def _report(rows, overflow=0, pool_cap=1000, locks=0, buckets=288):
    r = {k: 0 for k in SCALARS}
    r.update(rows=rows, overflow_entries=overflow, pool_cap=pool_cap, locks_held=locks, buckets=buckets, longest_chain_bucket=NO_BUCKET)
    r["chain_hist"], r["rows_hist"] = [0] * 17, [0] * 33
    return r


def test_needed_on_both_sides_of_each_threshold():
    adv = lambda *e, **kw: recovery.rehash_advice(list(e), **kw)  # noqa: E731
    # load: 288 buckets; 4.0 rows a bucket = 1152 rows
    assert not adv(_FakeEngine(W.STORE, 64, [_report(1152)]))["needed"]
    a = adv(_FakeEngine(W.STORE, 64, [_report(1153)]))
    assert a["needed"] and a["n_rows"] == recovery.advise_n_rows(W.STORE, [1153]) and a["load"] == [1153 / 288]
    assert not adv(_FakeEngine(W.STORE, 64, [_report(1153)]), max_rows_per_bucket=4.01)["needed"]
    # the pool: more than half of it linked
    assert not adv(_FakeEngine(W.STORE, 64, [_report(100, overflow=500)]))["needed"]
    assert adv(_FakeEngine(W.STORE, 64, [_report(100, overflow=501)]))["needed"]
    assert not adv(_FakeEngine(W.STORE, 64, [_report(100, overflow=501)]), max_pool_fill=0.6)["needed"]
    # a sharded set: the load is over the GLOBAL bucket count, the pool fill per engine
    two = [_FakeEngine(W.STORE, 64, [_report(576, buckets=144)]), _FakeEngine(W.STORE, 64, [_report(577, overflow=10, buckets=144)])]
    a = adv(*two)
    assert a["needed"] and a["tables"][0]["rows"] == 1153 and a["tables"][0]["buckets"] == 288
    two[1]._rep[0]["rows"] = 576
    assert not adv(*two)["needed"]
    two[0]._rep[0].update(overflow_entries=600)  # one engine's pool past the mark, the set's is not (610 of 2000)
    assert adv(*two)["needed"]
    # any table of several; locks are passed on
    t = [_report(100, buckets=750), _report(100), _report(100), _report(1875 * 4 + 1, locks=3), _report(0)]
    a = adv(_FakeEngine(W.TATP, 2000, t))
    assert a["needed"] and a["locks_held"] == 3 and a["n_rows"] == recovery.advise_n_rows(W.TATP, [r["rows"] for r in t])
    t[3]["rows"] -= 1
    assert not adv(_FakeEngine(W.TATP, 2000, t))["needed"]


if __name__ == "__main__":
    # the file the stand-alone sanitizer program reads: u64 images, then per image {u64 bytes, u64 tables, the image padded to 8
    # bytes, tables x 80 u64: the numpy form's report as dint_table_stats words}
    with open(sys.argv[1], "wb") as f:
        f.write(struct.pack("<Q", len(CASES)))
        for _, img in CASES:
            rep = np_image_stats(img)
            f.write(struct.pack("<QQ", img.nbytes, len(rep)))
            f.write(img.tobytes() + bytes(-img.nbytes % 8))
            for r in rep:
                f.write(struct.pack("<80Q", *([r[k] for k in SCALARS] + r["chain_hist"] + r["rows_hist"] + [0] * 13)))
    print(len(CASES), "images")
