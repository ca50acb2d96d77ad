"""One-pass traces whose HOT requests sit at chosen request indices (test tooling, numpy only; tests/test_gpu_hot_layout.py runs
them on the GPU, tests/test_hotlayout_host.py checks on the oracle and the rules below alone that every one of them holds what
it promises).

The kv and lock passes answer a hot key in closed form by cutting its requests along the request INDEX, so whether a rule of
that cutting is right depends on where the hot requests sit in the pass -- which no random trace varies.  A case here names the
indices and the op of every hot request; the other indices hold requests that never reach the hot sub or bin ("alone": log-type
requests for tatp / smallbank, which the partition finishes; bad-type requests for the store, echoed and counted; lids of other
bins for the lock tables), ordinary traffic on other keys ("traffic"), or the alone filler plus a handful of requests on a key of
the hot bucket ("neighbour").  In an alone case the hot sub holds exactly the hot key's records, the key the pieces are cut
around is the hot key with certainty (but for smallbank's cases with a foreign key on the row's counter pair: `kv_counters`), and
the engine's late counters follow from three rules restated here:

    np0 = ceil(h / target)                                          kv_list_items, k_kv_dev.h:2445
    hot iff h >= split_min and np0 <= np_max                        kv_list_items, k_kv_dev.h:2448
    piece_of(idx) = min(np - 1, (idx * np * (2^32 // n)) >> 32)     kv_piece_of,   k_kv_dev.h:2416-2419
    (split_min, target, np_max from the knobs: kv_read_knobs / kv_fill_pass, k_kv.hip:65-95, 145-156)

`kv_counters` turns a case's per-piece counts into the change of late_requests / late_items those rules imply.  The constants
(64, 384, 448, 512, 64 / 128 pieces, 8 foreign, 4096, 2048 buckets, 1024 rest records, 65,536) are read from the headers.

A case keeps its passes (the layout pass, then an ordinary pass on the same engine: the pieces' words are tagged per pass), the
oracle's replies and the oracle's final state; CASES names every case and the knob sets it runs under, `case(name)` builds one
and keeps the last few (the tests walk the cases in order)."""
from __future__ import annotations

import functools
import os
import re
from dataclasses import dataclass, field

import numpy as np

import kv_collide as kc
import kvkeys
import opwords as ow
import tracegen
from dint_amd import wire
from oracle import oracle as orc

W = wire.Workload
KV = (W.STORE, W.TATP, W.SMALLBANK)
CSRC = os.path.join(os.path.dirname(os.path.abspath(wire.__file__)), "csrc")


# ---- the constants, from the headers ----------------------------------------------------------------------------------------
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(text, pattern):
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(1))


_BINS, _KVDEV, _KV, _KVH, _LOCKS, _DEV = (_src(f) for f in ("dint_bins.h", "k_kv_dev.h", "k_kv.hip", "dint_kv.h", "k_locks.hip", "dint_device.h"))
KVB_T = _const(_BINS, r"#define KVB_T (\d+)u")                          # requests of one piece at most (a workgroup's threads)
KVB_NMAX = _const(_BINS, r"#define KVB_NMAX (\d+)u")                    # requests of one stretch
KVB_NBK = _const(_BINS, r"#define KVB_NBK (\d+)u")                      # request-index buckets that cut a bin into stretches
KVB_HOT_MIN = _const(_BINS, r"#define KVB_HOT_MIN (\d+)u")              # kv_big_bin's dominant-key threshold
KVB_HOT_MIN_LOCKS = _const(_BINS, r"#define KVB_HOT_MIN_LOCKS (\d+)u")  # ... the lock tables'
KVR_NPMAX = _const(_KVDEV, r"#define KVR_NPMAX (\d+)u")                 # pieces of a hot key, store / tatp
KSB_NPMAX = _const(_KVDEV, r"#define KSB_NPMAX (\d+)u")                 # ... smallbank
KSB_FMAX = _const(_KVDEV, r"#define KSB_FMAX (\d+)u")                   # foreign requests of one smallbank piece
KV_MMAX = _const(_KVDEV, r"constexpr uint32_t KV_MMAX = (\d+);")        # writers + lock ops of kv_big_bin's dominant key
BIG_SUB = _const(_KVDEV, r"bool big = h > (\d+);")                      # a sub of more records is a big sub (kv_coarse_bin)
SPLIT_MIN = _const(_KVH, r"uint32_t split_min = (\d+);")
SPLIT_TARGET = _const(_KVH, r"uint32_t split_target = (\d+);")
SB_SPLIT_MIN = _const(_KVH, r"uint32_t sb_split_min = (\d+);")
SB_NPMAX = _const(_KVH, r"uint32_t sb_npmax = (\d+);")
TARGET_MAX, TARGET_MIN = (int(x) for x in re.search(r"k\.split_target = std::min\((\d+)u, std::max\((\d+)u,", _KV).groups())
SPLIT_MIN_FLOOR = _const(_KV, r"k\.split_min = std::max\((\d+)u,")
SB_SPLIT_MIN_FLOOR = _const(_KV, r"A\.split_min = std::max\((\d+)u, K\.sb_split_min\)")
TPL_HOT_NMAX = _const(_LOCKS, r"#define TPL_HOT_NMAX (\d+)u")           # dominant-slot path: passes of at most this many requests
LK_BINCAP = _const(_DEV, r"#define DINT_KV_BINCAP (\d+)u")              # records a lock bin holds in place
LK_REST = KVB_NMAX // _const(_LOCKS, r"k_ < KVB_NMAX / (\d+)\) Rest\[k_\] = r")  # other records of the hot bin kept in LDS
LK_GROUP = 64                                                           # lock_2pl's mode walk: request indices per group (one 64-bit word)
assert (KVB_T, KVB_NMAX, KVB_NBK, KVR_NPMAX, KSB_NPMAX, KSB_FMAX, KV_MMAX, BIG_SUB, SPLIT_TARGET, TPL_HOT_NMAX, LK_REST) == \
    (512, 4096, 2048, 64, 128, 8, 2048, 64, 384, 65536, 1024), "the issue's figures: a changed constant wants its cases looked at again"

# knob sets (the hot-key tests' own: SPLIT_KNOBS / SB_KNOBS of tests/test_gpu_kv.py, by the ids used there) -> (environment, engine flags)
KNOBS = {
    "default": ({}, 0),
    "t16": ({"DINT_KV_SPLIT_MIN": "65", "DINT_KV_SPLIT_TARGET": "16"}, 0),
    "t100": ({"DINT_KV_SPLIT_MIN": "200", "DINT_KV_SPLIT_TARGET": "100"}, 0),
    "nosplit": ({"DINT_KV_NO_SPLIT": "1"}, 0),
    "late_big": ({"DINT_KV_LATE_BIG": "1"}, 0),
    "nofuse": ({"DINT_KV_NO_FUSE": "1"}, 0),
    "rounds": ({}, 1),  # DINT_FLAG_KV_ROUNDS: no closed form anywhere
    "sb-t64": ({"DINT_KV_SB_SPLIT_MIN": "200", "DINT_KV_SPLIT_TARGET": "64"}, 0),
    "sb-t300": ({"DINT_KV_SB_SPLIT_MIN": "600", "DINT_KV_SPLIT_TARGET": "300"}, 0),
    "sb-off": ({"DINT_KV_SB_SPLIT_MIN": "0"}, 0),
    "sb-min2048": ({"DINT_KV_SB_SPLIT_MIN": "2048"}, 0),
    "sb-big-only": ({"DINT_KV_SB_WORKERS": "0"}, 0),
    "lk-nodirect": ({"DINT_LOCK_NO_DIRECT": "1"}, 0),
    "lk-nofuse": ({"DINT_LOCK_NO_FUSE": "1"}, 0),
    "lk-min32": ({"DINT_LOCK_HOT_MIN": "32"}, 0),  # the dominant-slot path for a slot of 64 requests (one 64-index group)
    "lk-min32-nodirect": ({"DINT_LOCK_HOT_MIN": "32", "DINT_LOCK_NO_DIRECT": "1"}, 0),
}


# ---- the three rules ----------------------------------------------------------------------------------------------------------
def kv_rule(wl, knobs="default"):
    """(split_min, target, np_max) a pass of this engine lists its big subs with (kv_read_knobs, kv_fill_pass), None: no sub is
    ever listed as a solo item or as pieces (kv_uses_hot is false / smallbank's pieces are off)"""
    env, flags = KNOBS[knobs]
    get = lambda k, d: int(env.get(k, d))
    if (flags & 3) or get("DINT_KV_NO_SPLIT", 0):
        return None
    target = min(TARGET_MAX, max(TARGET_MIN, get("DINT_KV_SPLIT_TARGET", SPLIT_TARGET)))
    if wl == W.SMALLBANK:
        sm = get("DINT_KV_SB_SPLIT_MIN", SB_SPLIT_MIN)
        return (max(SB_SPLIT_MIN_FLOOR, sm), target, max(2, min(KSB_NPMAX, get("DINT_KV_SB_NPMAX", SB_NPMAX)))) if sm else None
    return max(SPLIT_MIN_FLOOR, get("DINT_KV_SPLIT_MIN", SPLIT_MIN)), target, KVR_NPMAX


def np0(h, target):
    return -(-h // target)


def listing(h, rule):
    """how kv_list_items lists a sub of h records: ("small", 0) -- no big sub, the chunk path; ("sub", 0) as it is; ("solo", 1);
    ("pieces", np)"""
    if h <= BIG_SUB:
        return "small", 0
    if rule is None:
        return "sub", 0
    split_min, target, np_max = rule
    n_p = np0(h, target)
    if not (h >= split_min and n_p <= np_max):
        return "sub", 0
    return ("solo", 1) if n_p == 1 else ("pieces", n_p)


def piece_of(idx, n_p, n):
    inv_n = (1 << 32) // n if n > 1 else 0xFFFFFFFF  # kv_fill_pass: A.inv_n
    p = (np.asarray(idx, np.uint64) * np.uint64(n_p) * np.uint64(inv_n)) >> np.uint64(32)
    return np.minimum(p, np.uint64(n_p - 1)).astype(np.int64)


@functools.lru_cache(64)
def ranges(n, n_p):
    """[(first, last)] request index of every piece's range R_0 .. R_np-1 of a pass of n"""
    p = piece_of(np.arange(n), n_p, n)
    first = np.searchsorted(p, np.arange(n_p), "left")
    last = np.searchsorted(p, np.arange(n_p), "right") - 1
    assert (last >= first).all() and first[0] == 0 and last[-1] == n - 1
    return list(zip(first.tolist(), last.tolist()))


def stretches(c, n):
    """stretches kv_big_bin / lk_big_bins cut c records of a pass of n into (k_kv_dev.h:1126-1128, 1160-1182; k_locks.hip:476-477, 739)"""
    if c <= KVB_NMAX:
        return 1
    nbits = (n - 1).bit_length() if n > 1 else 0
    bs = nbits - 11 if nbits > 11 else 0
    assert (1 << nbits) >> bs <= KVB_NBK
    return (c - 1) // (KVB_NMAX - (1 << bs)) + 1


def two_stretches_max(n):
    """the largest c that stretches(c, n) cuts in two"""
    nbits = (n - 1).bit_length()
    return 2 * (KVB_NMAX - (1 << (nbits - 11 if nbits > 11 else 0)))


# ---- ops --------------------------------------------------------------------------------------------------------------------------
# symbolic ops of a hot request: R read, W writer, A acquire, X abort / release, P commit-and-unlock, I / D insert / delete (tatp)
OPS = {
    W.STORE: {"R": 0, "W": 1, "A": 0, "X": 0, "P": 1},
    W.TATP: {"R": 0, "W": 13, "A": 1, "X": 2, "P": 12, "I": 18, "D": 22},
    W.SMALLBANK: {"R": 17, "W": 5, "A": 1, "X": 3, "P": 4, "S": 0, "s": 2},  # S / s: acquire / release shared
}
SIMPLE = {W.STORE: (0, 1), W.TATP: (0, 1, 2, 12, 13), W.SMALLBANK: (0, 1, 2, 3, 4, 5, 17)}  # kv_simple_op, k_kv_dev.h:586-590
WRITERS = {W.STORE: (1,), W.TATP: (12, 13), W.SMALLBANK: (4, 5)}                            # is_writer, kv_hot_item / kv_sb_item
LOCK_OPS = {W.STORE: (), W.TATP: (1, 2, 12, 18, 22), W.SMALLBANK: (0, 1, 2, 3)}             # kv_lock_op, k_kv_dev.h:602-606
FILLER = {W.STORE: 99, W.TATP: int(wire.Tatp.COMMIT_LOG), W.SMALLBANK: int(wire.Sb.COMMIT_LOG)}


def pattern(name, c):
    """c symbolic ops: "alt" writer / read alternating; "writers"; "locks" acquire / abort / commit-and-unlock around reads and
    writers; "reads+W@k": reads but one writer at rank k (negative: from the end)"""
    if name == "alt":
        return np.array(list("WR" * (c // 2 + 1))[:c])
    if name == "writers":
        return np.array(["W"] * c)
    if name == "locks":
        return np.array(list("ARWXRAPRW" * (c // 9 + 1))[:c])
    assert name.startswith("reads+W@"), name
    ops = np.array(["R"] * c)
    ops[int(name[8:])] = "W"
    return ops


def spread(lo, hi, k):
    """k distinct indices of [lo, hi], evenly spaced, lo and hi among them (k >= 2)"""
    assert 0 <= k <= hi - lo + 1, (lo, hi, k)
    if k == 0:
        return np.zeros(0, np.int64)
    if k == 1:
        return np.array([lo], np.int64)
    out = lo + (np.arange(k, dtype=np.int64) * (hi - lo)) // (k - 1)
    assert len(np.unique(out)) == k
    return out


# ---- a case ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Case(kc.Case):
    name: str = ""
    variant: str = "alone"             # alone / traffic / neighbour
    table: int = 0
    key: int = 0                       # the hot row, or the hot lid
    n: int = 0
    c: int = 0                         # requests of the hot key in pass 0
    built: str = "default"             # the knob set the layout is cut for
    promise: dict = field(default_factory=dict)  # what the layout says of itself under `built`: np, per piece / group counts, expect
    foreign: int = None                # smallbank: the other key on the hot row's counter pair
    bad: int = 0                       # store: bad-type requests (the alone filler), counted in bad_requests
    n_slots: int = 0                   # lock tables

    def lock_oracle(self):
        return orc.FasstOracle(self.n_slots) if self.wl == W.FASST else orc.TplOracle(self.n_slots)

    def replayed(self):
        if self.wl in KV:
            return super().replayed()
        o = self.lock_oracle()
        self.want = [o.replay(p) for p in self.passes]
        self.errors = o.errors
        a, b = (o.locks, o.vers) if self.wl == W.FASST else (o.num_ex, o.num_sh)
        self.locks = [(np.nonzero(x)[0], x[np.nonzero(x)[0]].copy()) for x in (a, b)]  # (sparse: a table of 2^20 slots, a few of them touched)
        return self


def same_rows(a, b):
    """two row dumps (keys, versions, values in bucket and chain order) are equal"""
    return all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


def row_exists(c: Case):
    """does the hot row exist in the populated tables, before any pass -- on a fresh oracle's dump"""
    o = c.oracle()
    keys = o.dump()[0] if c.wl == W.STORE else o.dump(c.table)[0]
    return bool((keys == np.uint64(c.key)).any())


def hot_sel(c: Case, k=0):
    p = c.passes[k]
    if c.wl in KV:
        sel = (p["key"] == np.uint64(c.key)) & (p["type"] != FILLER[c.wl])
        return sel & (p["table"] == c.table) if c.wl != W.STORE else sel
    return ow.lid_slot(p["lid"], c.n_slots) == int(ow.lid_slot([c.key], c.n_slots)[0])


def foreign_sel(c: Case, k=0):
    p = c.passes[k]
    return (p["key"] == np.uint64(c.foreign)) & (p["table"] == c.table) & (p["type"] != FILLER[c.wl]) if c.foreign is not None else np.zeros(len(p), bool)


def piece_counts(c: Case, knobs):
    """(listing kind, np, the hot pair's requests per piece, the foreign ones per piece) of pass 0 under a knob set -- from the
    trace and the rules alone.  The sub's records = the hot key's and (smallbank) the foreign key's: an alone case has no others."""
    hs, fs = hot_sel(c), foreign_sel(c)
    h = int(hs.sum() + fs.sum())
    kind, n_p = listing(h, kv_rule(c.wl, knobs))
    if n_p == 0:
        return kind, 0, [], []
    p = piece_of(np.arange(c.n), n_p, c.n)
    return kind, n_p, np.bincount(p[hs | fs], minlength=n_p).tolist(), np.bincount(p[fs], minlength=n_p).tolist()


def kv_counters(c: Case, knobs, around="hot"):
    """The change of (late_requests, late_items[0..2]) pass 0 of an ALONE case makes under a knob set, from the rules -- or None
    where they decide nothing (a solo item whose row is inserted or deleted: kv_solo_item's row machine).
    store / tatp (kv_hot_role, k_kv_dev.h:4014-4023): a big sub listed as it is is late as a whole, item kind 0; pieces of which one
    holds more than KVB_T requests or an op outside the closed form: piece 0 takes the key's records, item kind 2 (kv_hot_item,
    :3264, :3295, :3340-3362).  smallbank (kv_sb_item, :3723, :3754, :3767, :3876-3878): late_items[0] per piece over KVB_T,
    late_items[1] per piece over KSB_FMAX foreign requests, late_requests += the sub; a sub listed as it is counts nowhere.
    around="foreign" (a smallbank case with a foreign key): the counters when the pieces are cut around the FOREIGN key, which the
    vote of kv_list_items (k_kv_dev.h:2466-2483: a tie of eight samples falls to ONE record of the sub, whichever the partition's
    atomics put there) allows with probability the foreign key's share of the sub; the hot row's requests are then the foreign ones."""
    assert c.variant == "alone" and c.wl in KV
    kind, n_p, per, fper = piece_counts(c, knobs)
    h = int(hot_sel(c).sum() + foreign_sel(c).sum())
    types = c.passes[0]["type"][hot_sel(c) | foreign_sel(c)]
    simple = bool(np.isin(types, SIMPLE[c.wl]).all())
    zero = (0, [0, 0, 0])
    if kind == "small":
        return zero
    if c.wl == W.SMALLBANK:
        if kind == "sub":
            return zero
        if around == "foreign":
            assert c.foreign is not None
            fper = [a - b for a, b in zip(per, fper)]
        over, fover = sum(x > KVB_T for x in per), sum(x > KSB_FMAX for x in fper)
        return (h if over or fover else 0, [over, fover, 0])
    if kind == "sub":
        return (h, [1, 0, 0]) if kv_rule(c.wl, knobs) is not None else zero  # (no rule: k_kv_big takes every big sub, nothing is "late")
    if kind == "solo":
        return zero if simple else None
    return (h, [0, 0, 1]) if (max(per) > KVB_T or not simple) else zero


# ---- building kv cases ----------------------------------------------------------------------------------------------------------
N_SB = 2000
ROWS = {  # (table, key, exists)
    (W.STORE, "present"): (0, kc.STORE_HOT, True), (W.STORE, "absent"): (0, ow.STORE_HOT, False),
    (W.TATP, "present"): (0, 7, True), (W.TATP, "absent"): (0, 5_000_000, False), (W.TATP, "cf"): (4, 7 | (1 << 32), None),
    (W.SMALLBANK, "present"): (0, 7, True), (W.SMALLBANK, "absent"): (0, 900_000, False),
}


PASS_MAX = 1 << 20  # the engine's largest pass (engine.hip: DINT_KV_PASS) -- and never more than its log ring holds


def _engine_of(wl, n):
    """(Engine arguments, rows to populate, log ring entries): the ring holds the pass, or the engine would cut it in several"""
    log_cap = 1 << 16 if n <= 1 << 16 else PASS_MAX
    if wl == W.STORE:
        return dict(n_rows=kc.N_STORE), kc.N_STORE, 0
    if wl == W.TATP:
        return dict(n_rows=kc.N_SUB, log_entries=log_cap), kc.N_SUB, log_cap
    return dict(n_rows=N_SB, log_entries=log_cap), N_SB, log_cap


def _hash_size(wl, table):
    if wl == W.STORE:
        return kc.STORE_HS
    if wl == W.TATP:
        return kc.tatp_base()[1][table]
    return kc.sb_hs(N_SB)


def _filler(wl, n, seed):
    """n requests that never reach a sub: the store's are bad-type (echoed, counted), tatp's and smallbank's log-type (the partition
    appends them to the log and acks them)"""
    rng = np.random.default_rng(seed)
    m = np.zeros(n, wire.MSG_DTYPE[wl])
    m["type"] = FILLER[wl]
    m["key"] = rng.integers(0, 1 << 40, n, dtype=np.uint64)
    m["val"] = rng.integers(0, 256, m["val"].shape, dtype=np.uint8)
    m["ver"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype("<u4")
    if wl != W.STORE:
        m["ord"] = rng.integers(0, 256, n)
        m["table"] = rng.integers(0, 5 if wl == W.TATP else 2, n)
    return m


def _traffic(wl, n, seed, table, key):
    if wl == W.STORE:
        return kc.store_noise(n, seed, int(kvkeys.np_bucket([key], kc.STORE_HS)[0]))
    if wl == W.TATP:
        return kc.tatp_noise(n, seed, (kc.tatp_bucket_of(table, key),))
    return kc.sb_noise(n, seed, N_SB, (key,))


def _place(wl, req, idx, table, key, ops, tag):
    """the requests `idx` become `ops` (symbolic) on (table, key); every one carries a value and a version payload of its own"""
    idx = np.asarray(idx, np.int64)
    req["type"][idx] = [OPS[wl][o] for o in ops]
    req["key"][idx] = key
    if wl != W.STORE:
        req["table"][idx] = table
    val = np.zeros((len(idx), req["val"].shape[1]), np.uint8)
    val[:, :4] = np.frombuffer(idx.astype("<u4").tobytes(), np.uint8).reshape(-1, 4)  # (distinct: the request index ...)
    val[:, 4] = tag
    val[:, 5:8] = 0xA5
    req["val"][idx] = val
    req["ver"][idx] = (0x40000000 + (tag << 22) + idx).astype("<u4")  # ... and again in the version payload


def _second_pass(wl, table, key, seed, foreign=None):
    """an ordinary pass behind the layout: 1,500 requests, 40 % of them on the hot row, the rest traffic"""
    n = 1500
    req = _traffic(wl, n, seed, table, key)
    rng = np.random.default_rng(seed + 1)
    idx = np.nonzero(rng.random(n) < 0.4)[0]
    _place(wl, req, idx, table, key, rng.choice(list("RRRWAXP"), len(idx)), 3)
    if foreign is not None:
        f = rng.choice(np.setdiff1d(np.arange(n), idx), 5, replace=False)
        _place(wl, req, f, table, foreign, rng.choice(list("RWAX"), 5), 4)
    return req


def kv_case(wl, name, n, idx, ops, *, row="present", variant="alone", built="default", promise=None, foreign=None, seed=1):
    """pass 0: n requests, the ones at `idx` are `ops` on the hot row; `foreign` = (indices, ops) on the other key of the row's
    counter pair (smallbank)"""
    table, key, exists = ROWS[(wl, row)]
    idx = np.asarray(idx, np.int64)
    assert len(idx) == len(ops) and len(np.unique(idx)) == len(idx) and 0 <= idx.min() and idx.max() < n
    eng, pop, log_cap = _engine_of(wl, n)
    req = _traffic(wl, n, 7 + seed, table, key) if variant == "traffic" else _filler(wl, n, 7 + seed)
    _place(wl, req, idx, table, key, ops, 1)
    c = Case(wl, eng, pop, [req], log_cap=log_cap, name=name, variant=variant, table=table, key=key, n=n, c=len(idx), built=built,
             promise=dict({} if exists is None else {"exists": exists}, **(promise or {})))
    hs = _hash_size(wl, table)
    if foreign is not None:
        f_idx, f_ops = foreign
        c.foreign = int(kvkeys.keys_like(key, hs, 1, same_kh=True, same_quadrant=True, seed=18)[0])
        assert not np.isin(f_idx, idx).any()
        _place(wl, req, f_idx, table, c.foreign, f_ops, 2)
    if variant == "neighbour":  # six requests on two keys of the hot bucket behind OTHER key-hash bits: one in another lock quadrant, one in the same
        free = np.setdiff1d(np.arange(n), idx)
        at = free[spread(0, len(free) - 1, 6)]
        key_of = kvkeys.cf_key_of if (wl, row) == (W.TATP, "cf") else None
        for k, same_q in enumerate((False, True)):
            nb = int(kvkeys.keys_like(key, hs, 1, same_kh=False, same_quadrant=None if wl == W.STORE else same_q, seed=40 + k, key_of=key_of)[0])
            # (a lock op of a key on the hot key's lock byte refuses the closed form outright -- kv_hot_item's nbr check: the
            # neighbour of the same quadrant reads and writes only, so that the pieces and the remainder's vote are what runs)
            _place(wl, req, at[k::2], table, nb, list("RWR" if same_q else "RWA"), 5 + k)
    c.bad = int((req["type"] == 99).sum()) if wl == W.STORE else 0
    c.passes.append(_second_pass(wl, table, key, 100 + seed, c.foreign))
    return c.replayed()


# ---- the layouts: (n, hot indices, symbolic ops, promise) -----------------------------------------------------------------------
def _target(wl, built):
    return kv_rule(wl, built)[1]


def lay_even(wl, built, n, c, ops="alt"):
    return n, spread(0, n - 1, c), pattern(ops, c), {}


def lay_one_range(wl, built, n, c, which, ops="locks"):
    """front / back: all c in R_0 or in R_np-1, every other piece empty"""
    n_p = np0(c, _target(wl, built))
    lo, hi = ranges(n, n_p)[0 if which == "front" else n_p - 1]
    per = [0] * n_p
    per[0 if which == "front" else -1] = c
    return n, spread(lo, hi, c), pattern(ops, c), dict(np=n_p, per=per)


def lay_gap(wl, built, n, c):
    """only R_0 and R_np-1 are populated: the only writers and the only lock op in R_0, reads and one ACQUIRE in R_np-1"""
    n_p = np0(c, _target(wl, built))
    R = ranges(n, n_p)
    a = c // 2
    ops0 = pattern("alt", a)
    ops0[3] = "A"
    ops1 = np.array(["R"] * (c - a))
    ops1[(c - a) // 2] = "A"
    per = [0] * n_p
    per[0], per[-1] = a, c - a
    return n, np.concatenate([spread(*R[0], a), spread(*R[-1], c - a)]), np.concatenate([ops0, ops1]), dict(np=n_p, per=per)


def lay_full(wl, built, n, c, piece, count, ops="alt"):
    """`count` of the key's requests in R_piece, the rest spread over the other ranges"""
    n_p = np0(c, _target(wl, built))
    R = ranges(n, n_p)
    others = [j for j in range(n_p) if j != piece]
    share = [(c - count) // len(others) + (1 if k < (c - count) % len(others) else 0) for k in range(len(others))]
    per = [0] * n_p
    per[piece] = count
    for j, s in zip(others, share):
        per[j] = s
    idx = np.sort(np.concatenate([spread(*R[j], per[j]) for j in range(n_p)]))
    return n, idx, pattern(ops, c), dict(np=n_p, per=per)


def lay_all_full(wl, built, n, pieces_full):
    """KVB_T writers with distinct values in every populated piece: nwr = 512 in each word.  (np = ceil(c / target) and target <=
    448 < KVB_T, so c requests never fill ALL their np pieces: the pieces not in `pieces_full` are empty.)"""
    c = KVB_T * len(pieces_full)
    n_p = np0(c, _target(wl, built))
    R = ranges(n, n_p)
    per = [KVB_T if j in pieces_full else 0 for j in range(n_p)]
    idx = np.concatenate([spread(*R[j], KVB_T) for j in pieces_full])
    return n, idx, pattern("writers", c), dict(np=n_p, per=per)


def lay_straddle(wl, built, n, c, kind):
    """for every j: a request at the last index of R_j and one at the first of R_j+1 -- "wr": writer then READ, "rw": READ then
    writer, "ax": ACQUIRE / ABORT (alternating over j) then ACQUIRE; reads between them"""
    n_p = np0(c, _target(wl, built))
    R = ranges(n, n_p)
    per = [c // n_p + (1 if j < c % n_p else 0) for j in range(n_p)]
    idx, ops = [], []
    for j, (lo, hi) in enumerate(R):
        i = spread(lo, hi, per[j])
        o = np.array(["R"] * per[j])
        if j + 1 < n_p:
            o[-1] = {"wr": "W", "rw": "R", "ax": "AX"[j & 1]}[kind]
        if j > 0:
            o[0] = {"wr": "R", "rw": "W", "ax": "A"}[kind]
        idx.append(i); ops.append(o)
    edges = [(R[j][1], R[j + 1][0]) for j in range(n_p - 1)]
    return n, np.concatenate(idx), np.concatenate(ops), dict(np=n_p, per=per, edges=edges)


def lay_extremes(wl, built, n, c):
    """hot requests at index 0 and at n - 1, writers both (the last writer of the pass has the largest index there is)"""
    ops = pattern("alt", c)
    ops[-1] = "W"
    return n, spread(0, n - 1, c), ops, dict(first=0, last=n - 1)


def lay_cf(wl, built, n, c, piece):
    """tatp's CALL_FORWARDING row with its own DELETE and INSERT in R_piece only: the op outside the closed form, one piece
    refuses while its siblings are clean"""
    n_p = np0(c, _target(wl, built))
    R = ranges(n, n_p)
    per = [c // n_p + (1 if j < c % n_p else 0) for j in range(n_p)]
    idx = np.concatenate([spread(*R[j], per[j]) for j in range(n_p)])
    ops = pattern("locks", c)
    at = sum(per[:piece]) + per[piece] // 2
    exists = bool((kc.tatp_base()[0][4] == np.uint64(ROWS[(wl, "cf")][1])).any())
    ops[at], ops[at + 4] = ("D", "I") if exists else ("I", "D")
    return n, idx, ops, dict(np=n_p, per=per, struct_piece=piece, exists=exists)


def lay_mmax(wl, built, n, c, m):
    """c requests of the key, exactly m of them writers or lock ops (kv_big_bin's dominant-key path puts at most KV_MMAX in order)"""
    ops = np.array(["R"] * c)
    ops[spread(0, c - 1, m)] = np.array(list("WAXW" * (m // 4 + 1))[:m]) if wl != W.STORE else "W"
    return n, spread(0, n - 1, c), ops, dict(m=m)


def sb_foreign(built, n, c, f, where):
    """smallbank: c requests of the hot row spread evenly and f foreign ones (the other key of its counter pair) inside ONE range
    ("inside"), or one foreign request as the first / last index of a range"""
    n_p = np0(c + f, _target(W.SMALLBANK, built))
    R = ranges(n, n_p)
    j = n_p // 2
    lo, hi = R[j]
    f_idx = {"inside": spread(lo + 10, hi - 10, f) if f > 1 else np.array([lo + 10]), "first": np.array([lo]), "last": np.array([hi])}[where]
    assert len(f_idx) == f
    free = np.setdiff1d(np.arange(n), f_idx)
    idx = free[spread(0, len(free) - 1, c)]
    fper = [0] * n_p
    fper[j] = f
    return n, idx, pattern("locks", c), dict(np=n_p, fper=fper), (f_idx, np.array(list("AWXSRsAWX" * 2)[:f]))


# ---- lock tables ------------------------------------------------------------------------------------------------------------------
N_SLOTS = ow.N_SLOTS
LK_OPS = {"R": 0, "A": 1, "X": 2, "C": 3,                 # lock_fasst: READ, ACQUIRE, ABORT, COMMIT
          "s": (0, 0), "x": (0, 1), "r": (1, 0), "e": (1, 1), "u": (1, 7)}  # lock_2pl (action, type): acquire shared / exclusive, release shared / exclusive / of an unknown type (acked, changes nothing)


@functools.lru_cache(None)
def _lk_places():
    """(the hot lid, 15 lids on the OTHER slots of its 128-byte line -- the hot bin's other records --, filler lids whose line
    numbers differ from the hot line's in their low five bits).  A lock bin is the low pbits bits of the 16-slot line number
    (lk_count_body, k_locks.hip:165), and pbits >= 5 for a pass of more than 512 requests (dint_pick_bins_kv): no filler shares
    the hot bin, whatever the pass size."""
    first, _ = ow.lid_maps()
    hot = ow.HOT_LID
    hs = int(ow.lid_slot([hot])[0])
    line = [s for s in range(hs & ~15, (hs & ~15) + 16) if s != hs and first[s] != 0]
    assert len(line) == 15
    lids = np.arange(1, 400_001, dtype=np.uint32)
    fill = lids[((ow.lid_slot(lids) >> 4) & 31) != ((hs >> 4) & 31)]
    return hot, first[np.array(line)].astype(np.uint32), fill


def _lk_msgs(wl, lids, ops, seed):
    m = np.zeros(len(lids), wire.MSG_DTYPE[wl])
    m["lid"] = lids
    if wl == W.FASST:
        m["type"] = [LK_OPS[o] for o in ops]
        m["ver"] = np.random.default_rng(seed).integers(0, 1 << 32, len(lids), dtype=np.uint64).astype("<u4")
    else:
        at = np.array([LK_OPS[o] for o in ops], np.uint8).reshape(-1, 2)
        m["action"], m["type"] = at[:, 0], at[:, 1]
    return m


def lk_case(wl, name, n, idx, ops, *, variant="alone", rest=0, built="default", promise=None, max_pass=0, seed=1):
    """pass 0: n requests, the ones at `idx` are `ops` on the hot lid; `rest` more on the other slots of the hot slot's line (the hot
    bin's other records); the others on lids of other bins, a few each ("alone"), or tracegen's random traffic ("traffic")"""
    hot, line, fill = _lk_places()
    idx = np.asarray(idx, np.int64)
    assert len(idx) == len(ops) and len(np.unique(idx)) == len(idx) and idx.max() < n
    rng = np.random.default_rng(seed)
    alphabet = list("RAXC") if wl == W.FASST else list("sxre")
    if variant == "traffic":
        req = (tracegen.fasst_random if wl == W.FASST else tracegen.tpl_random)(n, seed=seed, n_hot=64, p_hot=0.3)
    else:
        req = _lk_msgs(wl, fill[rng.integers(0, len(fill), n)], rng.choice(alphabet, n), seed)
    req[idx] = _lk_msgs(wl, np.full(len(idx), hot, np.uint32), ops, seed + 1)
    if rest:
        free = np.setdiff1d(np.arange(n), idx)
        at = free[spread(0, len(free) - 1, rest)]
        req[at] = _lk_msgs(wl, line[np.arange(rest) % len(line)], rng.choice(alphabet, rest), seed + 2)
    c = Case(wl, dict(n_slots=N_SLOTS, **({"max_pass": max_pass} if max_pass else {})), 0, [req], name=name, variant=variant, key=hot, n=n,
             c=len(idx), built=built, promise=dict(promise or {}, rest=rest), n_slots=N_SLOTS)
    n2 = 3000  # the ordinary pass behind it: random traffic, a third of it on the hot lid
    req2 = (tracegen.fasst_random if wl == W.FASST else tracegen.tpl_random)(n2, seed=seed + 3, n_hot=64, p_hot=0.3)
    req2["lid"][rng.random(n2) < 0.33] = hot
    c.passes.append(req2)
    return c.replayed()


def lk_ops(wl, name, c):
    """c ops on the hot slot.  "mix": every op in turn; "commits": lock_fasst COMMITs only; "acq-abort": ACQUIRE / ABORT alternating;
    "shared": lock_2pl shared acquires and releases (the mode never changes)"""
    if name == "commits":
        return np.array(["C"] * c)
    if name == "acq-abort":
        return np.array(list("AX" * (c // 2 + 1))[:c])
    if name == "shared":
        return np.array(list("ssr" * (c // 3 + 1))[:c])
    word = "ARCXRAARC" if wl == W.FASST else "ssxrreexsr"
    return np.array(list(word * (c // len(word) + 1))[:c])


def lk_groups(wl, n, groups, per_group, ops="mix"):
    """the hot slot's requests in the 64-index groups `groups`, per_group of them in each"""
    idx = np.concatenate([spread(LK_GROUP * g, min(n, LK_GROUP * (g + 1)) - 1, per_group) for g in groups])
    return n, idx, lk_ops(wl, ops, len(idx)), dict(groups=list(groups), per_group=per_group)


def lk_mode_edge(n, c, edge, order="sx"):
    """lock_2pl: shared traffic everywhere, and a mode change across the indices edge - 1 / edge, the groups 64 k - 1 | 64 k.  "sx":
    the last shared holder releases at edge - 1, an exclusive acquire at edge is granted, its release and a shared acquire follow;
    "xs": the exclusive acquire is granted at edge - 1 and HOLDS across the edge (a shared acquire at edge is rejected), released at
    edge + 1, a shared acquire at edge + 2 is granted"""
    idx = np.unique(np.concatenate([spread(0, n - 1, c - 6), [edge - 3, edge - 2, edge - 1, edge, edge + 1, edge + 2]]))
    ops = np.array(["s"] * len(idx))
    # before the edge every shared acquire is released again, so that edge - 1 is the release of the LAST holder
    below = np.nonzero(idx < edge - 3)[0]
    ops[below[1::2]] = "r"
    if len(below) % 2:
        ops[below[-1]] = "u"
    at = {int(i): k for k, i in enumerate(idx)}
    for i, o in zip(range(edge - 3, edge + 3), "sxrxes" if order == "sx" else "srxses"):  # "sx": shared acquire, exclusive rejected, the shared release | exclusive granted, released, shared
        ops[at[i]] = o
    return n, idx, ops, dict(edge=edge, order=order)


# ---- every case, by name: (builder, knob sets it runs under; the first is `built`) ---------------------------------------------------
CASES = {}


def _kv(name, wl, lay, *, row="present", variants=("alone",), knobs=("default",), **kw):
    for v in variants:
        def make(v=v, nm=f"{name}-{v}"):
            out = lay(wl, knobs[0])
            foreign = out[4] if len(out) > 4 else None
            return kv_case(wl, nm, out[0], out[1], out[2], row=row, variant=v, built=knobs[0], promise=out[3], foreign=foreign, **kw)
        CASES[f"{name}-{v}"] = (make, tuple(knobs) if v == "alone" else tuple(knobs[:1]))


def _lk(name, wl, lay, *, variants=("alone",), knobs=("default", "lk-nodirect"), **kw):
    for v in variants:
        def make(v=v, nm=f"{name}-{v}"):
            n, idx, ops, promise = lay()
            return lk_case(wl, nm, n, idx, ops, variant=v, built=knobs[0], promise=promise, **kw)
        CASES[f"{name}-{v}"] = (make, tuple(knobs) if v == "alone" else tuple(knobs[:1]))


ALL3 = ("alone", "traffic", "neighbour")
P = functools.partial
_WL = {"store": W.STORE, "tatp": W.TATP}
for _w, _wl in _WL.items():
    _nof = ("default", "t100", "nosplit", "nofuse", "rounds")
    _kv(f"{_w}-even", _wl, P(lay_even, n=4096, c=1500), variants=ALL3, knobs=_nof)
    for _k, _at in (("first", 0), ("last", -1), ("middle", 750)):
        _kv(f"{_w}-one-writer-{_k}", _wl, P(lay_even, n=4096, c=1500, ops=f"reads+W@{_at}"), knobs=("default", "t16" if _k == "middle" else "t100"))
    _kv(f"{_w}-even-absent", _wl, P(lay_even, n=4096, c=1500, ops="locks"), row="absent", knobs=("default", "t16"))
    for _which in ("front", "back"):
        _kv(f"{_w}-{_which}", _wl, P(lay_one_range, n=16384, c=KVB_T, which=_which), variants=ALL3, knobs=("t16", "late_big"))
        _kv(f"{_w}-{_which}-np2", _wl, P(lay_one_range, n=4096, c=KVB_T, which=_which), knobs=("default",))
    _kv(f"{_w}-gap-np3", _wl, P(lay_gap, n=4096, c=800), variants=ALL3, knobs=("default", "nofuse"))
    _kv(f"{_w}-gap-np64", _wl, P(lay_gap, n=32768, c=1024), variants=ALL3, knobs=("t16", "late_big"))
    _kv(f"{_w}-gap-np64-absent", _wl, P(lay_gap, n=32768, c=1024), row="absent", knobs=("t16",))
    _kv(f"{_w}-full-512", _wl, P(lay_full, n=4096, c=1500, piece=1, count=KVB_T), variants=ALL3, knobs=("default", "late_big", "nofuse"))
    _kv(f"{_w}-full-513", _wl, P(lay_full, n=4096, c=1500, piece=1, count=KVB_T + 1), variants=ALL3, knobs=("default", "late_big", "nofuse"))
    _kv(f"{_w}-full-513-absent", _wl, P(lay_full, n=4096, c=1500, piece=2, count=KVB_T + 1, ops="locks"), row="absent", knobs=("default",))
    _kv(f"{_w}-all-full-absent", _wl, P(lay_all_full, n=4096, pieces_full=(0, 2, 3)), row="absent", knobs=("default",))
    _kv(f"{_w}-full-513-last", _wl, P(lay_full, n=4096, c=1500, piece=3, count=KVB_T + 1, ops="locks"), knobs=("default",))
    _kv(f"{_w}-full-512-t16", _wl, P(lay_full, n=32768, c=1000, piece=40, count=KVB_T, ops="locks"), knobs=("t16",))
    _kv(f"{_w}-all-full", _wl, P(lay_all_full, n=4096, pieces_full=(0, 1, 3)), variants=ALL3, knobs=("default", "nofuse"))
    _kv(f"{_w}-seven-full", _wl, P(lay_all_full, n=8192, pieces_full=(0, 1, 2, 3, 4, 5, 6)), knobs=("default",))
    for _kind in ("wr", "rw", "ax"):
        _kv(f"{_w}-straddle-{_kind}", _wl, P(lay_straddle, n=4096, c=128, kind=_kind), variants=ALL3 if _kind == "wr" else ("alone",), knobs=("t16", "nofuse"))
        _kv(f"{_w}-straddle-{_kind}-np64", _wl, P(lay_straddle, n=5000, c=1024, kind=_kind), knobs=("t16",))
    _kv(f"{_w}-straddle-wr-absent", _wl, P(lay_straddle, n=4096, c=128, kind="wr"), row="absent", knobs=("t16",))
    _kv(f"{_w}-extremes-2^19", _wl, P(lay_extremes, n=1 << 19, c=1024), knobs=("default",))
    _kv(f"{_w}-extremes-2^19+1", _wl, P(lay_extremes, n=(1 << 19) + 1, c=1024), knobs=("default",))
    _kv(f"{_w}-extremes-2^20", _wl, P(lay_extremes, n=1 << 20, c=1024), knobs=("t16",))
    for _c in (BIG_SUB, BIG_SUB + 1, SPLIT_TARGET, SPLIT_TARGET + 1):
        _kv(f"{_w}-count-{_c}", _wl, P(lay_even, n=4096, c=_c, ops="locks"), knobs=("default", "nofuse"))
    for _c in (KVR_NPMAX * SPLIT_TARGET, KVR_NPMAX * SPLIT_TARGET + 1):
        _kv(f"{_w}-count-{_c}", _wl, P(lay_even, n=32768, c=_c), knobs=("default",))
    for _c in (KVB_HOT_MIN - 1, KVB_HOT_MIN, KVB_HOT_MIN + 1, KVB_NMAX - 1, KVB_NMAX, KVB_NMAX + 1, two_stretches_max(16384), two_stretches_max(16384) + 1):
        _kv(f"{_w}-nosplit-count-{_c}", _wl, P(lay_even, n=16384, c=_c, ops="locks"), knobs=("nosplit",))
    for _m in (KV_MMAX, KV_MMAX + 1):
        _kv(f"{_w}-nosplit-ordering-{_m}", _wl, P(lay_mmax, n=8192, c=4000, m=_m), knobs=("nosplit",))
_kv("tatp-cf-even", W.TATP, P(lay_even, n=4096, c=1500, ops="locks"), row="cf", variants=ALL3, knobs=("default", "t16"))
_kv("tatp-cf-own-insert-in-one-piece", W.TATP, P(lay_cf, n=4096, c=1500, piece=2), row="cf", variants=ALL3, knobs=("default", "t100", "nofuse"))
_kv("tatp-cf-own-insert-in-piece-0", W.TATP, P(lay_cf, n=4096, c=1500, piece=0), row="cf", knobs=("default",))

_SB = W.SMALLBANK
_sbk = ("default", "sb-t64", "sb-t300", "sb-off", "sb-min2048", "sb-big-only", "nofuse", "rounds")
_kv("smallbank-even", _SB, P(lay_even, n=4096, c=1500, ops="locks"), variants=ALL3, knobs=_sbk)
for _k, _at in (("first", 0), ("last", -1)):
    _kv(f"smallbank-one-writer-{_k}", _SB, P(lay_even, n=4096, c=1500, ops=f"reads+W@{_at}"), knobs=("default", "sb-t64"))
_kv("smallbank-even-absent", _SB, P(lay_even, n=4096, c=1500, ops="locks"), row="absent", knobs=("default", "sb-t64"))
for _which in ("front", "back"):
    _kv(f"smallbank-{_which}", _SB, P(lay_one_range, n=16384, c=KVB_T, which=_which), variants=ALL3, knobs=("sb-t64", "sb-big-only"))
_kv("smallbank-gap-np3", _SB, P(lay_gap, n=4096, c=800), variants=ALL3, knobs=("default", "nofuse"))
_kv("smallbank-gap-np16", _SB, P(lay_gap, n=16384, c=1024), variants=ALL3, knobs=("sb-t64", "sb-big-only"))
_kv("smallbank-gap-np64", _SB, P(lay_gap, n=32768, c=1024), variants=ALL3, knobs=("t16",))  # (the coordinator walks 62 empty pieces)
_kv("smallbank-gap-np64-absent", _SB, P(lay_gap, n=32768, c=1024), row="absent", knobs=("t16",))
_kv("smallbank-full-512", _SB, P(lay_full, n=4096, c=1500, piece=1, count=KVB_T, ops="locks"), variants=ALL3, knobs=("default", "sb-big-only", "nofuse"))
_kv("smallbank-full-513", _SB, P(lay_full, n=4096, c=1500, piece=1, count=KVB_T + 1, ops="locks"), variants=ALL3, knobs=("default", "sb-big-only", "nofuse"))
_kv("smallbank-all-full", _SB, P(lay_all_full, n=4096, pieces_full=(0, 1, 3)), variants=ALL3, knobs=("default", "nofuse"))
for _kind in ("wr", "rw", "ax"):
    _kv(f"smallbank-straddle-{_kind}", _SB, P(lay_straddle, n=4096, c=1024, kind=_kind), variants=ALL3 if _kind == "wr" else ("alone",), knobs=("sb-t64", "nofuse"))
    _kv(f"smallbank-straddle-{_kind}-np64", _SB, P(lay_straddle, n=5000, c=1024, kind=_kind), knobs=("t16",))
_kv("smallbank-extremes-2^19", _SB, P(lay_extremes, n=1 << 19, c=1024), knobs=("default",))
_kv("smallbank-extremes-2^19+1", _SB, P(lay_extremes, n=(1 << 19) + 1, c=1024), knobs=("default",))
_kv("smallbank-extremes-2^20", _SB, P(lay_extremes, n=1 << 20, c=1024), knobs=("sb-t64",))
for _c in (BIG_SUB, BIG_SUB + 1, SPLIT_TARGET, SPLIT_TARGET + 1):
    _kv(f"smallbank-count-{_c}", _SB, P(lay_even, n=4096, c=_c, ops="locks"), knobs=("default", "sb-big-only"))
for _c in (KSB_NPMAX * SPLIT_TARGET, KSB_NPMAX * SPLIT_TARGET + 1):
    _kv(f"smallbank-count-{_c}", _SB, P(lay_even, n=65536, c=_c, ops="locks"), knobs=("default",))
for _c in (KVB_HOT_MIN - 1, KVB_HOT_MIN, KVB_HOT_MIN + 1, KVB_NMAX - 1, KVB_NMAX, KVB_NMAX + 1, two_stretches_max(16384), two_stretches_max(16384) + 1):
    _kv(f"smallbank-off-count-{_c}", _SB, P(lay_even, n=16384, c=_c, ops="locks"), knobs=("sb-off",))
# (the foreign key wins the vote for the key the pieces are cut around when the ONE sampled record that decides a tie is its own:
# 9 records of 40,009 -- kv_list_items, k_kv_dev.h:2466-2483; then the hot row is the foreign one and the sub is refused: the
# candidate key of these cases is NOT certain, and the GPU test accepts kv_counters(around="foreign") beside the usual outcome)
for _f, _where in ((KSB_FMAX, "inside"), (KSB_FMAX + 1, "inside"), (1, "first"), (1, "last")):
    _kv(f"smallbank-foreign-{_f}-{_where}", _SB, lambda wl, built, f=_f, where=_where: sb_foreign(built, 65536, 40_000, f, where),
        knobs=("default", "sb-big-only", "nofuse"))

for _w, _wl in (("fasst", W.FASST), ("2pl", W.TPL)):
    _NG = TPL_HOT_NMAX // LK_GROUP
    _lk(f"{_w}-one-group", _wl, P(lk_groups, _wl, TPL_HOT_NMAX, (500,), LK_GROUP), rest=10, knobs=("lk-min32", "lk-min32-nodirect"), variants=("alone", "traffic"))
    _lk(f"{_w}-one-per-group", _wl, P(lk_groups, _wl, TPL_HOT_NMAX, range(_NG), 1), variants=("alone", "traffic"), knobs=("default", "lk-nodirect", "lk-nofuse"))
    _lk(f"{_w}-first-and-last-group", _wl, P(lk_groups, _wl, TPL_HOT_NMAX, (0, _NG - 1), LK_GROUP), knobs=("lk-min32", "lk-min32-nodirect"), variants=("alone", "traffic"))
    _lk(f"{_w}-first-and-last-group-full", _wl, P(lk_groups, _wl, TPL_HOT_NMAX, (0, 1, 2, _NG - 3, _NG - 2, _NG - 1), LK_GROUP))
    for _r in (LK_REST, LK_REST + 1):
        _lk(f"{_w}-rest-{_r}", _wl, P(lk_groups, _wl, TPL_HOT_NMAX, range(0, _NG, 8), 20), rest=_r, variants=("alone", "traffic"))
    for _c in (KVB_HOT_MIN_LOCKS - 1, KVB_HOT_MIN_LOCKS, KVB_HOT_MIN_LOCKS + 1, LK_BINCAP, LK_BINCAP + 1):
        _lk(f"{_w}-count-{_c}", _wl, P(lambda wl, c: (8192, spread(0, 8191, c), lk_ops(wl, "mix", c), {}), _wl, _c))
    _lk(f"{_w}-above-65536", _wl, P(lambda wl: ((1 << 17) + 5, spread(0, 1 << 17, 9000), lk_ops(wl, "mix", 9000), {}), _wl), max_pass=1 << 20,
        knobs=("default", "lk-nodirect"))
_lk("fasst-65536-commits", W.FASST, P(lk_groups, W.FASST, TPL_HOT_NMAX, range(TPL_HOT_NMAX // LK_GROUP), LK_GROUP, "commits"), knobs=("default", "lk-nodirect", "lk-nofuse"))
_lk("fasst-65536-acquire-abort", W.FASST, P(lk_groups, W.FASST, TPL_HOT_NMAX, range(TPL_HOT_NMAX // LK_GROUP), LK_GROUP, "acq-abort"))
for _e in (64, 4096):
    _lk(f"2pl-mode-change-at-{_e - 1}|{_e}", W.TPL, P(lk_mode_edge, 8192, 600, _e), variants=("alone", "traffic"))
    _lk(f"2pl-exclusive-held-across-{_e - 1}|{_e}", W.TPL, P(lk_mode_edge, 8192, 600, _e, "xs"))


@functools.lru_cache(3)
def case(name) -> Case:
    return CASES[name][0]()


def runs():
    """every (case name, knob set) the GPU test runs, a case's knob sets side by side"""
    return [(name, k) for name, (_, knobs) in CASES.items() for k in knobs]
