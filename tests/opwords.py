"""Every short op word on ONE slot or row, from every start state, as traces for the parity tests (test tooling, numpy only;
tests/test_gpu_opwords.py runs them on the GPU, tests/test_opwords_host.py checks on the host that they hold what they promise).

A word is a sequence of ops of one workload's alphabet on one lock slot / one row.  A start is the state the word is answered
from (lock free or held, counters 0 / 1 / 2, row present / absent / held twice).  Two kinds of trace:

cold   every (start, word) with 1 <= len(word) <= Lc on a slot or key of its own: one submit of all preambles, then the words
       adjacent (word after word) or transposed (op 0 of every word, then op 1 of every word ...).  Layouts: "spread" (own lock
       words), "lockpair" (tatp / smallbank: two words on two keys of one bucket AND lock quadrant), "alias" / "line" (locks: two
       words on two lids of one slot / on neighbouring slots of one 128-byte line).  For sets of H sharded engines
       (tests/shardsplit.py) two more, placed by the shard geometry: "edge" (cold_edge) and "localline" (cold_localline).
hot    every (start, word) with len(word) == Lh on ONE slot or row, block after block: preamble(start) + word + cleanup.  The
       trace is built against a live oracle: after the word the oracle's state of the slot is read and the ops that lead back to
       idle are emitted (releases, ABORT, INSERT / DELETE until the row is what the next start wants); the oracle's replies along
       the way are the expected output, there is no second model of the semantics.  Words that leave a state no op leaves (an
       exclusive counter wrapped by an unmatched release; a store row that was to stay absent and got inserted) are found from the
       cold replay and put at the END, in blocks without cleanup, followed by one de Bruijn sequence of order Lh over the alphabet:
       the wrapped region on purpose.  `dilute` puts d requests on other slots / keys between every two of a hot trace, `dual`
       runs a hot trace and its rotation on two keys of one lock word (or two lids of one line) at once.

The row multiplicity of a kv key is read as the oracle's row count less the count at the start (nothing else is inserted or
deleted while a trace is built) and checked against o.dump at the end; smallbank rows can be neither inserted nor deleted, so its
present / absent starts are two traces on two keys; smallbank's "both" target sends every op to the SAVING and then to the
CHECKING row of the account, so both rows go through every word.

Sizes as built (tests/test_opwords_host.py prints them):

  workload   target           Lc  cold words  cold requests   Lh  hot requests  front blocks  tail blocks
  lock_fasst slot              5        7810          37110    5         39598          6250            0
  lock_2pl   slot              4        6216          23640    4         31761          3134         2050
  store      row               6       10920          61896    6         53254          4825         3367
  tatp       subscriber        3       11304          32904    3         46920         10368            0
  tatp       call_forwarding   3       11304          32904    3         46921         10368            0
  smallbank  saving            3        6552          18864    3         15199          2263          653
  smallbank  both              3        6552          37728    3         30398          2263          653
  (smallbank hot: the same sizes with the row present and with the row absent)
"""
from __future__ import annotations

import collections
import functools
import itertools
from dataclasses import dataclass, field

import numpy as np

import kvkeys
import tracegen
from dint_amd import wire
from oracle import oracle as orc
from shard_double import fasthash_lid

W = wire.Workload
COLD_MAX, HOT_MAX = 65_536, 60_000
POP, POP_BIG, LOG_CAP, N_SLOTS = 3000, 24_000, 400_000, 1 << 20
HOT_LID, SB_ABSENT = 777, 900_000
TATP_HOT = {"subscriber": (0, 7), "call_forwarding": (4, 7 | (1 << 32))}
STORE_HOT = int(tracegen.store_key(77_777, 1, 0))  # no populated row
U32 = 1 << 32


@dataclass(frozen=True)
class Spec:
    name: str
    wl: object
    alphabet: tuple    # op codes: the request type; lock_2pl: action << 4 | type
    starts: tuple
    targets: tuple
    hot_order: tuple = None   # the order of the starts in a hot trace (store: a row cannot be made absent again)


def _grid(a, b):
    return tuple(f"{x}-{y}" for x in a for y in b)


COUNTERS = ("idle", "sh1", "sh2", "ex1")
SPECS = {
    "lock_fasst": Spec("lock_fasst", W.FASST, (0, 1, 2, 3, 200), ("free", "held"), ("slot",)),
    "lock_2pl": Spec("lock_2pl", W.TPL, (0x00, 0x01, 0x10, 0x11, 0x09, 0x19), COUNTERS, ("slot",)),
    "store": Spec("store", W.STORE, (0, 1, 2, 77), ("present", "absent"), ("row",), ("absent", "present")),
    "tatp": Spec("tatp", W.TATP, (0, 1, 2, 3, 12, 13, 14, 18, 19, 22, 23, 24), _grid(("present", "absent", "twice"), ("free", "held")),
                 ("subscriber", "call_forwarding")),
    "smallbank": Spec("smallbank", W.SMALLBANK, (0, 1, 2, 3, 4, 5, 6, 17, 99), _grid(COUNTERS, ("present", "absent")), ("saving", "both")),
}
_COUNTER_STATE = {"idle": (0, 0), "sh1": (0, 1), "sh2": (0, 2), "ex1": (1, 0)}  # (exclusive, shared)
_ROWS = {"present": 1, "absent": 0, "twice": 2}
# the ops that move a state: (acquire shared, acquire exclusive, release shared, release exclusive)
_COUNTER_OPS = {W.TPL: (0x00, 0x01, 0x10, 0x11), W.SMALLBANK: (0, 1, 2, 3)}


def is_lock(spec):
    return spec.wl in (W.FASST, W.TPL)


def layouts(spec):
    """the key layouts of a workload's cold traces"""
    return ("spread", "alias", "line") if is_lock(spec) else ("spread",) if spec.wl == W.STORE else ("spread", "lockpair")


def tables_of(spec, target):
    if spec.wl == W.TATP:
        return (TATP_HOT[target][0],)
    if spec.wl == W.SMALLBANK:
        return (0, 1) if target == "both" else (0,)
    return (0,)


def start_state(spec, start):
    """the slot state a start names: fasst (lock,), 2pl / smallbank (exclusive, shared), store (rows,), tatp (rows, lock byte)"""
    if spec.wl == W.FASST:
        return (int(start == "held"),)
    if spec.wl == W.TPL:
        return _COUNTER_STATE[start]
    if spec.wl == W.STORE:
        return (_ROWS[start],)
    a, b = start.split("-")
    if spec.wl == W.TATP:
        return (_ROWS[a], int(b == "held"))
    return _COUNTER_STATE[a]


def idle_state(spec, start):
    """the state between two blocks: locks free, counters zero, the row as `start` wants it"""
    s = start_state(spec, start)
    if spec.wl == W.STORE:
        return s
    if spec.wl == W.TATP:
        return (s[0], 0)
    return (0,) * len(s)


def in_state(spec, state, want):
    if spec.wl == W.STORE:  # a store row cannot be deleted: present is one row or more
        return (state[0] > 0) == (want[0] > 0)
    return tuple(state) == tuple(want)


def fix_ops(spec, cur, want):
    """the op codes that take the slot from state `cur` to state `want`, or None where no op sequence does"""
    if in_state(spec, cur, want):
        return []
    if spec.wl == W.FASST:
        return [1] if want[0] else [2]
    if spec.wl == W.STORE:
        return [2] if want[0] else None
    if spec.wl == W.TATP:
        (rows, lock), (w_rows, w_lock) = cur, want
        ops = [2] if lock else []
        ops += [19] * (w_rows - rows) + [23] * (rows - w_rows)  # INSERT_BCK / DELETE_BCK leave the lock byte alone
        return ops + ([1] if w_lock else [])
    acq_sh, acq_ex, rel_sh, rel_ex = _COUNTER_OPS[spec.wl]
    ex, sh = cur
    if ex >= U32 // 2:  # an exclusive counter wrapped by an unmatched release: nothing is granted on this slot again
        return None
    ops = [rel_ex] * ex
    ops += [acq_sh] * (U32 - sh) if sh >= U32 // 2 else [rel_sh] * sh  # a wrapped shared counter comes back by granted acquires
    return ops + [acq_ex] * want[0] + [acq_sh] * want[1]


def words(spec, length):
    return list(itertools.product(spec.alphabet, repeat=length))


def de_bruijn(k: int, n: int) -> list:
    """one linear de Bruijn sequence of order n over range(k): k ** n + n - 1 symbols, every n-window once"""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
            return
        a[t] = a[t - p]
        db(t + 1, p)
        for j in range(a[t - p] + 1, k):
            a[t] = j
            db(t + 1, t)

    db(1, 1)
    return seq + seq[:n - 1]


# ---- requests -------------------------------------------------------------------------------------------------------------------
def blank(spec, n, seed):
    """n requests with random payload (val, ver, ord): the payload must not influence a reply code"""
    rng = np.random.default_rng(seed)
    m = np.zeros(n, wire.MSG_DTYPE[spec.wl])
    if "ver" in m.dtype.names:
        m["ver"] = rng.integers(0, U32, n, dtype=np.uint64).astype("<u4")
    if "val" in m.dtype.names:
        m["val"] = rng.integers(0, 256, (n,) + m.dtype["val"].shape, dtype=np.uint8)
    if "ord" in m.dtype.names:
        m["ord"] = rng.integers(0, 256, n)
    return m


def set_ops(spec, m, codes):
    codes = np.asarray(codes, np.uint8)
    if spec.wl == W.TPL:
        m["action"], m["type"] = codes >> 4, codes & 15
    else:
        m["type"] = codes


def set_place(spec, m, table, key):
    if is_lock(spec):
        m["lid"] = key
    else:
        m["key"] = key
        if spec.wl != W.STORE:
            m["table"] = table


def requests(spec, codes, tables, keys, seed):
    m = blank(spec, len(codes), seed)
    set_ops(spec, m, codes)
    set_place(spec, m, tables, keys)
    return m


def reply_pairs(spec, req, rep):
    """(request type, reply code) of every request; lock_2pl: (action, type, reply code)"""
    if spec.wl == W.TPL:
        return list(zip(req["action"].tolist(), req["type"].tolist(), rep["action"].tolist()))
    return list(zip(req["type"].tolist(), rep["type"].tolist()))


# ---- oracles and engines ----------------------------------------------------------------------------------------------------------
def sizes(spec, big=False):
    """(rows or accounts the tables are sized for, rows populated)"""
    if spec.wl == W.STORE:
        return (POP_BIG, POP) if big else (POP, POP)
    return (POP_BIG, POP_BIG) if big else (POP, POP)


def oracle(spec, big=False, n_slots=N_SLOTS):
    n, pop = sizes(spec, big)
    if spec.wl == W.FASST:
        return orc.FasstOracle(n_slots)
    if spec.wl == W.TPL:
        return orc.TplOracle(n_slots)
    if spec.wl == W.STORE:
        return orc.StoreOracle(n * 18 // 4, pop)
    if spec.wl == W.TATP:
        return orc.TatpOracle(n, log_entries=LOG_CAP, populate_n=pop)
    return orc.SmallbankOracle(n, log_entries=LOG_CAP, populate_n=pop)


def engine_args(spec, big=False, n_slots=N_SLOTS):
    """(keyword arguments of Engine, rows to populate)"""
    n, pop = sizes(spec, big)
    if is_lock(spec):
        return dict(n_slots=n_slots), 0
    if spec.wl == W.STORE:
        return dict(n_rows=n), pop
    return dict(n_rows=n, log_entries=LOG_CAP), pop


def lock_word(keys, hash_size):
    """index of the lock byte / counter pair of every key: fasthash64(key) % (4 * hash_size)"""
    b, q, _ = kvkeys.key_sig(keys, hash_size)
    return (q * np.uint64(hash_size) + b).astype(np.int64)


def lid_slot(lids, n_slots=N_SLOTS):
    return (fasthash_lid(np.atleast_1d(np.asarray(lids, np.uint32))) % np.uint64(n_slots)).astype(np.int64)


def _row_count(spec, o, table):
    L = orc.lib()
    if spec.wl == W.STORE:
        return L.orc_kvs_count(L.orc_store_table(o.h))
    return L.orc_kvs_count(L.orc_tatp_table(o.h, table))


def _rows_of(spec, o, table, key):
    keys = o.dump()[0] if spec.wl == W.STORE else o.dump(table)[0]
    return int((keys == np.uint64(key)).sum())


class Probe:
    """reads the oracle's state of one slot or row.  by_dump: the rows of a kv key are counted in o.dump, what the host tests check
    the traces with; else from the table's row count (module docstring), what a builder can afford block by block"""

    def __init__(self, spec, o, table, key, n_slots=N_SLOTS, by_dump=False):
        self.spec, self.o, self.table, self.key, self.by_dump = spec, o, table, key, by_dump
        if is_lock(spec):
            self.at = int(lid_slot([key], n_slots)[0])
        elif spec.wl != W.STORE:
            self.at = int(lock_word([key], o.hash_size(table))[0])
        if spec.wl in (W.STORE, W.TATP) and not by_dump:
            self.rows0 = _rows_of(spec, o, table, key) - _row_count(spec, o, table)

    def rows(self):
        if self.by_dump:
            return _rows_of(self.spec, self.o, self.table, self.key)
        return self.rows0 + _row_count(self.spec, self.o, self.table)

    def state(self):
        s, o = self.spec, self.o
        if s.wl == W.FASST:
            return (int(o.locks[self.at]),)
        if s.wl == W.TPL:
            return (int(o.num_ex[self.at]), int(o.num_sh[self.at]))
        if s.wl == W.STORE:
            return (self.rows(),)
        if s.wl == W.TATP:
            return (self.rows(), int(o.locks(self.table)[self.at]))
        return (int(o.num_ex(self.table)[self.at]), int(o.num_sh(self.table)[self.at]))


def slot_state(spec, o, table, key, n_slots=N_SLOTS):
    """the state of one slot or row of any oracle, rows counted in o.dump"""
    return Probe(spec, o, table, key, n_slots, by_dump=True).state()


# ---- cold -------------------------------------------------------------------------------------------------------------------------
def cold_preamble(spec, start):
    """the ops that set a start up on a fresh table (kv: a populated row for every start but smallbank's `absent`; store: a fresh key)"""
    return fix_ops(spec, (0,) if spec.wl == W.STORE else (1, 0) if spec.wl == W.TATP else idle_state(spec, start), start_state(spec, start))


def cold_length(spec, target):
    """Lc: the longest words for which one batch of all (start, word) stays within COLD_MAX requests"""
    rep, a, s = len(tables_of(spec, target)), len(spec.alphabet), len(spec.starts)
    L, total = 0, 0
    while total + rep * s * a ** (L + 1) * (L + 1) <= COLD_MAX:
        L += 1
        total += rep * s * a ** L * L
    return L


def _spaced(x, n):
    assert len(x) >= n, (len(x), n)
    return x[:: len(x) // n][:n]


def _lock_pairs(keys, hash_size):
    """pairs of `keys` on one lock word (one bucket AND one lock quadrant), no key twice"""
    lw = lock_word(keys, hash_size)
    o = np.argsort(lw, kind="stable")
    sl, sk = lw[o], np.asarray(keys, np.uint64)[o]
    first = np.nonzero((sl[1:] == sl[:-1]) & np.concatenate([[True], sl[1:-1] != sl[:-2]]))[0]  # the first two keys of a word
    return np.stack([sk[first], sk[first + 1]], axis=1)


def _lock_groups(keys, hash_size):
    """the keys whose lock word holds two or more of `keys`, keys of one lock word side by side"""
    lw = lock_word(keys, hash_size)
    o = np.argsort(lw, kind="stable")
    sl, sk = lw[o], np.asarray(keys, np.uint64)[o]
    same = sl[1:] == sl[:-1]
    return sk[np.concatenate([same, [False]]) | np.concatenate([[False], same])]


def _own_lock_words(keys, hash_size):
    lw = lock_word(keys, hash_size)
    return np.asarray(keys, np.uint64)[np.sort(np.unique(lw, return_index=True)[1])]


@functools.lru_cache(None)
def lid_maps():
    lids = np.arange(1, 8_000_001, dtype=np.uint32)
    slot = lid_slot(lids)
    o = np.argsort(slot, kind="stable")
    ss, sl = slot[o], lids[o]
    head = np.concatenate([[True], ss[1:] != ss[:-1]])
    first = np.zeros(N_SLOTS, np.uint32)
    first[ss[head]] = sl[head]
    two = np.nonzero(head[:-1] & ~head[1:])[0]  # slots with two lids or more: the first two
    return first, np.stack([sl[two], sl[two + 1]], axis=1)


def _lid_places(layout, n):
    first, alias = lid_maps()
    if layout == "spread":
        return _spaced(first[first != 0], n)
    if layout == "alias":
        return _spaced(alias, (n + 1) // 2).ravel()[:n]
    s = np.arange(0, N_SLOTS, 2)  # "line": slots 2k and 2k + 1 lie in one 128-byte line of 16 slots
    s = s[(first[s] != 0) & (first[s + 1] != 0)]
    s = _spaced(s, (n + 1) // 2)
    return np.stack([first[s], first[s + 1]], axis=1).ravel()[:n]


def _kv_places(spec, target, layout, presence):
    """one key per word; presence[i]: the word's row is to exist before its preamble (smallbank's absent rows never do)"""
    n, table = len(presence), tables_of(spec, target)[0]
    rng = np.random.default_rng(21)
    if spec.wl == W.STORE:
        return np.unique(rng.integers(1 << 50, 1 << 62, 2 * n, dtype=np.uint64))[:n]
    o = oracle(spec, big=True)
    hs = o.hash_size(table)
    pools = {True: np.sort(o.dump(table)[0])}
    if spec.wl == W.SMALLBANK:
        pools[False] = np.unique(rng.integers(1 << 33, 1 << 48, 200_000, dtype=np.uint64))
    out = np.zeros(n, np.uint64)
    if layout == "spread":
        both = _own_lock_words(np.concatenate([pools[k] for k in sorted(pools, reverse=True)]), hs)  # (the populated rows first)
        for k, pool in pools.items():
            sel = np.nonzero(presence == k)[0]
            out[sel] = _spaced(both[np.isin(both, pool)], len(sel))
        return out
    assert layout == "lockpair", layout
    for k, pool in pools.items():
        sel = np.nonzero(presence == k)[0]
        pairs = _lock_pairs(pool, hs)
        if 2 * len(pairs) >= len(sel):
            out[sel] = _spaced(pairs, (len(sel) + 1) // 2).ravel()[:len(sel)]
        else:  # too few pairs among the populated rows: every key whose lock word holds two or more of them, word by word
            out[sel] = _lock_groups(pool, hs)[:len(sel)]
    return out


@dataclass
class Cold:
    spec: Spec
    target: str
    layout: str
    L: int
    blocks: list                 # (start, word) per word, in trace order
    keys: np.ndarray             # the lid / key of every word
    pre: np.ndarray = None       # the first submit: every word's preamble
    adjacent: np.ndarray = None
    transposed: np.ndarray = None
    block_of: dict = field(default_factory=dict)  # arrangement -> the word of every request
    tables: np.ndarray = None    # layout "edge": the table of every word (the other layouts: the target's tables)
    pairs: list = None           # the shard-aware layouts: (kind, shard, word a, word b) of every pair that shares what `kind` says

    def final_states(self):
        """the oracle's state of every word's slot after preamble + word (layout "spread": every word from its true start)"""
        o = oracle(self.spec, big=True)
        o.replay(self.pre)
        o.replay(self.adjacent)
        return self.states(o)

    def states(self, o, table=None):
        """oracle o's state of every word's slot (of the target's first table)"""
        spec = self.spec
        table = tables_of(spec, self.target)[0] if table is None else table
        if is_lock(spec):
            at = lid_slot(self.keys)
            cols = (o.locks[at],) if spec.wl == W.FASST else (o.num_ex[at], o.num_sh[at])
        elif spec.wl == W.SMALLBANK:
            at = lock_word(self.keys, o.hash_size(table))
            cols = (o.num_ex(table)[at], o.num_sh(table)[at])
        else:
            keys, cnt = np.unique(o.dump()[0] if spec.wl == W.STORE else o.dump(table)[0], return_counts=True)
            i = np.minimum(np.searchsorted(keys, self.keys), len(keys) - 1)
            cols = (np.where(keys[i] == self.keys, cnt[i], 0),)
            if spec.wl == W.TATP:
                cols += (o.locks(table)[lock_word(self.keys, o.hash_size(table))],)
        return [tuple(int(c[i]) for c in cols) for i in range(len(self.keys))]


@functools.lru_cache(None)
def cold(name, target, layout="spread") -> Cold:
    spec = SPECS[name]
    L = cold_length(spec, target)
    tabs = tables_of(spec, target)
    blocks = [(s, w) for s in spec.starts for k in range(1, L + 1) for w in words(spec, k)]
    if is_lock(spec):
        keys = _lid_places(layout, len(blocks))
    else:
        keys = _kv_places(spec, target, layout, np.array([not s.endswith("-absent") for s, _ in blocks]))
    assert len(np.unique(keys)) == len(blocks)
    c = Cold(spec, target, layout, L, blocks, keys)

    def build(ops_of, transposed, seed):
        """requests of ops_of(word index) for every word: word after word, or op k of every word for k = 0, 1, ..."""
        rows = [(k, i, op) for i in range(len(blocks)) for k, op in enumerate(ops_of(i))]
        if transposed:
            rows.sort(key=lambda r: r[0])  # (stable: words stay in order within an op index)
        idx = np.repeat(np.array([r[1] for r in rows], np.int64), len(tabs))
        codes = np.repeat(np.array([r[2] for r in rows], np.int64), len(tabs))
        return requests(spec, codes, np.tile(np.array(tabs), len(rows)), keys[idx], seed), idx

    c.pre, c.block_of["pre"] = build(lambda i: cold_preamble(spec, blocks[i][0]), False, 31)
    c.adjacent, c.block_of["adjacent"] = build(lambda i: blocks[i][1], False, 32)
    c.transposed, c.block_of["transposed"] = build(lambda i: blocks[i][1], True, 32)
    assert len(c.adjacent) <= COLD_MAX
    return c


# ---- cold, placed by the geometry of a set of H shards ---------------------------------------------------------------------------------
# Shard g % H is home to global bucket / slot g and holds it at local index g // H; every shard's tables have n_local = ceil(size / H)
# local buckets, kv group keys are gk_base[t] + local with gk_base summed from the n_local values, kv lock words sit at
# q * n_local + local.  "edge" (kv) and "localline" (locks) put words where that arithmetic has its edges.
def _arranged(c: Cold, pre_of, tabs_of):
    """fill c.pre / adjacent / transposed as cold() does, word i on the tables tabs_of(i) (all of one length)"""
    spec, keys, blocks = c.spec, c.keys, c.blocks

    def build(ops_of, transposed, seed):
        rows = [(k, i, op) for i in range(len(blocks)) for k, op in enumerate(ops_of(i))]
        if transposed:
            rows.sort(key=lambda r: r[0])
        rep = len(tabs_of(0))
        idx = np.repeat(np.array([r[1] for r in rows], np.int64), rep)
        codes = np.repeat(np.array([r[2] for r in rows], np.int64), rep)
        tabs = np.array([tabs_of(r[1]) for r in rows], np.int64).ravel()
        return requests(spec, codes, tabs, keys[idx], seed), idx

    c.pre, c.block_of["pre"] = build(pre_of, False, 41)
    c.adjacent, c.block_of["adjacent"] = build(lambda i: blocks[i][1], False, 42)
    c.transposed, c.block_of["transposed"] = build(lambda i: blocks[i][1], True, 42)
    return c


def kv_hash_sizes(spec, big=False):
    if spec.wl == W.STORE:
        return [sizes(spec, big)[0] * 18 // 4]
    o = oracle(spec, big)
    return [int(o.hash_size(t)) for t in range(5 if spec.wl == W.TATP else 2)]


def edge_places(hash_sizes, H):
    """(table, shard) of every shard whose TOP local bucket n_local - 1 of the table corresponds to a global bucket (the greatest
    the shard is home to): there group key gk_base[t] + n_local - 1 is followed by gk_base[t + 1] + 0, the shard's local bucket 0
    (global bucket = shard index) of the next table"""
    return [(t, i) for t, hs in enumerate(hash_sizes) for i in range(H) if -(-hs // H) >= 2 and (-(-hs // H) - 1) * H + i < hs]


EDGE_PER = 4  # keys per (bucket, lock quadrant) of a top bucket: 16 rows in that bucket at the most


@functools.lru_cache(None)
def cold_edge(name, H) -> Cold:
    """layout "edge": pairs of words, for every place (t, i) of edge_places and every lock quadrant q, on
      cross     a key of shard i's top bucket of table t, quadrant q | a key of global bucket i of table t + 1 (the shard's local
                bucket 0 there), quadrant q: neighbours in group-key space, so a coarse bin can hold the end of one table and the
                start of the next;
      wrap      the last table (store: the only one): the top bucket | the least local bucket of the same table;
      quadrant  a second key of the top bucket, quadrant q | a key of local bucket 0 of table t, quadrant q + 1: for q = 0..2 their
                lock words q * n_local + n_local - 1 and (q + 1) * n_local are neighbours (q = 3 pairs with quadrant 0).
    The keys are searched, not populated (tables of the small size, where H = 2 and H = 8 leave remainders in every table): a
    word's preamble INSERTs its row where the start wants one; smallbank's rows cannot be inserted, so its words start from the
    `absent` starts alone.  There are as many words as places: all of length 1 and an evenly spaced sample of the longer ones."""
    spec = SPECS[name]
    hs = kv_hash_sizes(spec)
    places = edge_places(hs, H)
    o = oracle(spec) if spec.wl != W.STORE else None
    top = lambda t, i: (-(-hs[t] // H) - 1) * H + i  # noqa: E731
    T, B = {}, {}
    for t in range(len(hs)):
        taken = np.zeros(0, np.uint64) if o is None else o.dump(t)[0]
        mine = [i for tt, i in places if tt == t]
        below = sorted({i for tt, i in places if tt in (t, t - 1)})  # local bucket 0: the partner of table t's and of table t - 1's tops
        cells = [(top(t, i), q) for i in mine for q in range(4)] + [(i, q) for i in below for q in range(4)]
        if not cells:
            continue
        k = kvkeys.keys_in_cells(hs[t], cells, 2 * EDGE_PER, 60 + t, exclude=taken)
        for (b, q), row in zip(cells[:4 * len(mine)], k):
            T[t, b % H, q] = row
        for (b, q), row in zip(cells[4 * len(mine):], k[4 * len(mine):]):
            B[t, b, q] = row
    slots, pairs = [], []  # (table, key) of every word; the pairs
    for t, i in places:
        for q in range(4):
            for k in range(EDGE_PER):
                if k % 2:
                    kind, other = "quadrant", (t, int(B[t, i, (q + 1) % 4][k]))
                elif t + 1 < len(hs):
                    kind, other = "cross", (t + 1, int(B[t + 1, i, q][k]))
                else:
                    kind, other = "wrap", (t, int(B[t, i, q][EDGE_PER + k]))
                pairs.append((kind, i, len(slots), len(slots) + 1))
                slots += [(t, int(T[t, i, q][k])), other]
    n = len(slots)
    starts = tuple(s for s in spec.starts if spec.wl != W.SMALLBANK or s.endswith("-absent"))
    L = cold_length(spec, spec.targets[0])
    one = [(s, w) for s in starts for w in words(spec, 1)]
    more = [(s, w) for s in starts for k in range(2, L + 1) for w in words(spec, k)]
    assert n > len(one), (n, len(one))
    blocks = one + _spaced(more, n - len(one))
    rng = np.random.default_rng(5)
    blocks = [blocks[j] for j in rng.permutation(n)]  # (no op length or start tied to a kind of place)
    c = Cold(spec, "edge", "edge", L, blocks, np.array([k for _, k in slots], np.uint64), tables=np.array([t for t, _ in slots]), pairs=pairs)
    assert len(np.unique(c.keys)) == n
    absent = (0,) if spec.wl == W.STORE else (0, 0)
    pre = (lambda b: cold_preamble(spec, blocks[b][0])) if spec.wl == W.SMALLBANK else (lambda b: fix_ops(spec, absent, start_state(spec, blocks[b][0])))
    return _arranged(c, pre, lambda b: (int(c.tables[b]),))


def _localline_lids(n, H):
    first, _ = lid_maps()
    per = -(-((n + 1) // 2) // H)
    out = []
    for i in range(H):  # global slots g and g + H of home i: locals l and l + 1, l even and both on one line of 16 slots
        g = np.arange(i, N_SLOTS - H, H)
        g = g[((g // H) % 2 == 0) & (first[g] != 0) & (first[g + H] != 0)]
        last = i + (N_SLOTS - 1 - i) // H * H
        g = _spaced(g[(g != i) & (g != last) & (g + H != last)], per)
        assert first[last] and first[i], (i, last)
        out.append(np.concatenate([[[first[last], first[i]]], np.stack([first[g], first[g + H]], axis=1)]))  # (the last local slot | local 0)
    return np.stack(out, axis=1).reshape(-1, 2)  # pair k of shard 0, of shard 1 ... pair k + 1 of shard 0


@functools.lru_cache(None)
def cold_localline(name, H) -> Cold:
    """layout "localline": every word of cold(), pairs of words on two lids of ONE home whose LOCAL slots are neighbours on one
    128-byte line of that shard's table -- global slots g and g + H, which the unsharded engine holds H slots apart; the first pair
    of every shard on the shard's last local slot and its local slot 0"""
    spec = SPECS[name]
    L = cold_length(spec, "slot")
    blocks = [(s, w) for s in spec.starts for k in range(1, L + 1) for w in words(spec, k)]
    lids = _localline_lids(len(blocks), H)
    m = len(blocks) // 2
    pairs = [("ends" if k < H else "line", k % H, 2 * k, 2 * k + 1) for k in range(m)]
    c = Cold(spec, "slot", "localline", L, blocks, lids.ravel()[:len(blocks)].astype(np.uint32), pairs=pairs)
    assert len(np.unique(c.keys)) == len(blocks)
    return _arranged(c, lambda b: cold_preamble(spec, blocks[b][0]), lambda b: (0,))


# ---- hot --------------------------------------------------------------------------------------------------------------------------
@dataclass
class Hot:
    spec: Spec
    target: str
    L: int
    table: int
    key: int
    req: np.ndarray
    want: np.ndarray             # the replies the live oracle gave while the trace was built
    blocks: list                 # (start, word): n_front blocks with cleanup, then the tail
    n_front: int
    block_off: np.ndarray        # first request of every block (its preamble), then the de Bruijn sequence, then len(req)
    word_off: np.ndarray         # first request of every block's word
    errors: int = 0

    @property
    def n_tail(self):
        return len(self.blocks) - self.n_front

    def block_at(self, i):
        """the block request i belongs to: (index, start, word), or a name for what lies outside the blocks"""
        b = int(np.searchsorted(self.block_off, i, side="right")) - 1
        if b < 0:
            return "lead-in"
        if b >= len(self.blocks):
            return "de Bruijn sequence"
        return (b, "front" if b < self.n_front else "tail") + self.blocks[b]


def hot_starts(spec, present=True):
    order = spec.hot_order or spec.starts
    if spec.wl == W.SMALLBANK:
        return tuple(s for s in order if s.endswith("-present" if present else "-absent"))
    return order


def hot_length(spec, target, present=True):
    """the longest words whose blocks alone (no preamble, no cleanup) stay below HOT_MAX requests: an upper bound of Lh"""
    rep, a, s = len(tables_of(spec, target)), len(spec.alphabet), len(hot_starts(spec, present))
    L = 1
    while rep * (s * a ** (L + 1) * (L + 1) + a ** (L + 1)) < HOT_MAX:
        L += 1
    return L


def hot_place(spec, target, present=True):
    if is_lock(spec):
        return 0, HOT_LID
    if spec.wl == W.STORE:
        return 0, STORE_HOT
    if spec.wl == W.TATP:
        return TATP_HOT[target]
    return 0, (7 if present else SB_ABSENT)


class _TooLong(Exception):
    pass


def _build_hot(spec, target, present, L) -> Hot:
    tabs = tables_of(spec, target)
    rep = len(tabs)
    table, key = hot_place(spec, target, present)
    starts = hot_starts(spec, present)
    c = cold(spec.name, target)
    final = {b: s for b, s in zip(c.blocks, c.final_states())}
    every = [(s, w) for s in starts for w in words(spec, L)]
    ok = [fix_ops(spec, final[b], idle_state(spec, b[0])) is not None for b in every]
    front = [b for b, k in zip(every, ok) if k]
    tail = [b for b, k in zip(every, ok) if not k]

    o = oracle(spec)
    probes = [Probe(spec, o, t, key) for t in tabs]
    pool = blank(spec, 2 * HOT_MAX + 4096, 7 + L)
    set_place(spec, pool, np.tile(np.array(tabs), len(pool) // rep), key)
    want = np.zeros_like(pool)
    pos = 0

    def emit(codes):
        nonlocal pos
        n = rep * len(codes)
        if pos + n > len(pool):
            raise _TooLong
        set_ops(spec, pool[pos:pos + n], np.repeat(np.asarray(codes, np.int64), rep))
        want[pos:pos + n] = o.replay(pool[pos:pos + n])
        pos += n

    def state():
        s = [p.state() for p in probes]
        assert all(x == s[0] for x in s), s  # (smallbank "both": the two rows go in step)
        return s[0]

    block_off, word_off = [], []
    emit(fix_ops(spec, state(), idle_state(spec, front[0][0])))  # the lead-in: the row as the first start wants it
    for i, (start, word) in enumerate(front):
        assert in_state(spec, state(), idle_state(spec, start)), (i, start, word, state())
        block_off.append(pos)
        emit(fix_ops(spec, state(), start_state(spec, start)))
        assert in_state(spec, state(), start_state(spec, start)), (i, start, word, state())
        word_off.append(pos)
        emit(word)
        back = fix_ops(spec, state(), idle_state(spec, front[min(i + 1, len(front) - 1)][0]))
        assert back is not None and len(back) <= 16, (i, start, word, state())
        emit(back)
    for start, word in tail:  # from whatever state the earlier ones left: the start's own ops, the word, no cleanup
        block_off.append(pos)
        emit(cold_preamble(spec, start))
        word_off.append(pos)
        emit(word)
    block_off.append(pos)
    emit([spec.alphabet[k] for k in de_bruijn(len(spec.alphabet), L)])
    block_off.append(pos)
    if spec.wl in (W.STORE, W.TATP):
        assert probes[0].rows() == _rows_of(spec, o, table, key)
    return Hot(spec, target, L, table, key, pool[:pos].copy(), want[:pos].copy(), front + tail, len(front),
               np.array(block_off), np.array(word_off), int(getattr(o, "errors", 0)))


@functools.lru_cache(None)
def hot(name, target, present=True) -> Hot:
    """Lh is the largest length for which the whole trace stays below HOT_MAX requests"""
    spec = SPECS[name]
    L = hot_length(spec, target, present)
    while True:
        try:
            h = _build_hot(spec, target, present, L)
            if len(h.req) < HOT_MAX:
                return h
        except _TooLong:
            pass
        L -= 1


# ---- diluted, and two hot traces at once --------------------------------------------------------------------------------------------
def fillers(spec, n, seed, avoid_key):
    """n requests that leave every other slot or row as it is: READs of existing keys (smallbank: WARMUP_READ); lock_2pl:
    shared-acquire-and-release pairs on other slots"""
    rng = np.random.default_rng(seed)
    if is_lock(spec):
        lids = _lid_places("spread", 64)
        if spec.wl == W.FASST:
            return requests(spec, np.zeros(n, np.int64), 0, lids[rng.integers(0, 64, n)], seed)
        j = np.arange(n)
        return requests(spec, np.where(j % 2 == 0, 0x00, 0x10), 0, lids[(j // 2) % 64], seed)
    s_id = rng.integers(0, POP - 1, n).astype(np.uint64)
    s_id += s_id >= np.uint64(avoid_key & 0xFFFFFFFF)  # (not the hot subscriber / account)
    if spec.wl == W.STORE:
        return requests(spec, np.zeros(n, np.int64), 0, tracegen.store_key(s_id, rng.integers(1, 5, n), rng.integers(0, 3, n) * 8), seed)
    if spec.wl == W.TATP:
        return requests(spec, np.zeros(n, np.int64), 0, s_id, seed)
    return requests(spec, np.full(n, 17), rng.integers(0, 2, n), s_id, seed)


def dilute(h: Hot, d: int):
    """(requests, src): d fillers between every two requests of h; src[i] = the request of h at i, or -1"""
    n = len(h.req)
    out = np.zeros(n + (n - 1) * d, h.req.dtype)
    src = np.full(len(out), -1, np.int64)
    at = np.arange(n) * (d + 1)
    out[at], src[at] = h.req, np.arange(n)
    out[src < 0] = fillers(h.spec, int((src < 0).sum()), 50 + d, h.key)
    return out, src


def interleave(a, b, ratio):
    """ratio requests of a, one of b, and so on; what is left of either at the end; (requests, source, index in the source)"""
    n = min(len(a) // ratio, len(b))
    who = np.concatenate([np.tile(np.array([0] * ratio + [1]), n), np.zeros(len(a) - n * ratio, np.int64), np.ones(len(b) - n, np.int64)])
    out = np.zeros(len(who), a.dtype)
    out[who == 0], out[who == 1] = a, b
    idx = np.zeros(len(who), np.int64)
    idx[who == 0], idx[who == 1] = np.arange(len(a)), np.arange(len(b))
    return out, who, idx


@functools.lru_cache(None)
def dual_keys(name):
    """two populated tatp subscribers / smallbank accounts on one lock word (one bucket, one quadrant); two lids on neighbouring
    slots of one 128-byte line"""
    spec = SPECS[name]
    if is_lock(spec):
        return tuple(int(x) for x in _lid_places("line", 2))
    hs = oracle(spec).hash_size(0)
    return tuple(int(x) for x in _lock_pairs(np.arange(POP, dtype=np.uint64), hs)[0])


def localline_dual_lids(H):
    """two lids of one home of a set of H lock shards on neighbouring LOCAL slots of one 128-byte line: global slots g and g + H"""
    return tuple(int(x) for x in _localline_lids(4 * H, H)[H])  # (the pairs in front are the shards' last slot | slot 0)


def dual(name, target, ratio, keys=None):
    """the hot trace on one key and the same trace rotated by half its blocks on the other, interleaved ratio : 1.  The per-block
    start states do not hold here; the expected replies are one oracle replay of the whole.  keys: dual_keys(name) unless given"""
    spec = SPECS[name]
    h = hot(name, target)
    ka, kb = keys or dual_keys(name)
    cut = int(h.block_off[len(h.blocks) // 2])
    a, b = h.req.copy(), np.concatenate([h.req[cut:], h.req[:cut]])
    set_place(spec, a, a["table"] if "table" in a.dtype.names else 0, ka)
    set_place(spec, b, b["table"] if "table" in b.dtype.names else 0, kb)
    out, who, idx = interleave(a, b, ratio)
    src = np.where(who == 0, idx, (idx + cut) % len(h.req))
    return out, src


# ---- expected replies, computed once ------------------------------------------------------------------------------------------------
_EXPECTED = collections.OrderedDict()


def expected(tag, make_oracle, passes):
    """(replies pass by pass, the oracle afterwards -- to be read, not replayed further), kept per `tag`: the last twelve, since an
    oracle holds its tables and a log ring"""
    if tag not in _EXPECTED:
        o = make_oracle()
        _EXPECTED[tag] = ([o.replay(p) for p in passes], o)
        while len(_EXPECTED) > 12:
            _EXPECTED.popitem(last=False)
    _EXPECTED.move_to_end(tag)
    return _EXPECTED[tag]


def first_difference(got, want, block_at=None):
    """None, or (index of the first request whose reply differs, the block it belongs to, the two replies)"""
    item = want.dtype.itemsize
    x, y = np.frombuffer(got.tobytes(), "u1"), np.frombuffer(want.tobytes(), "u1")
    if len(x) != len(y):
        return ("length", len(x) // item, len(y) // item)
    bad = np.nonzero(x != y)[0]
    if not len(bad):
        return None
    i = int(bad[0]) // item
    g = np.frombuffer(got.tobytes(), want.dtype)
    return (i, block_at(i) if block_at else None, g[i].tolist(), want[i].tolist())
