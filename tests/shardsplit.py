"""The projection of an UNSHARDED oracle onto the shards of a set (test tooling, numpy only; tests/test_gpu_shard_words.py runs
sets of sharded engines against it, tests/test_shardsplit_host.py shows on the oracle alone that it holds what it promises).

A set is H engines, shard i of H.  With g = the global bucket (kv: fasthash64(key) % hash_size of the table) or the global slot
(locks: fasthash64(lid) % n_slots) of a request, shard g % H is its home and g // H its local bucket / slot there.  A table of
`size` global buckets has n_local = ceil(size / H) local ones on EVERY shard; on the shards i with (n_local - 1) * H + i >= size
the top local bucket corresponds to no global one and must stay empty.  kv lock words sit at q * n_local + local (q = the lock
quadrant), not at lock_hash.

Expected values of a set that is sent a trace, every request to its home:
  replies            one unsharded oracle replay of the whole trace (requests of different buckets commute, so a shard that sees
                     only its own answers them as the one server does);
  rows, lock words   that oracle's final state, projected (project_rows / project_kv_locks / project_slots);
  ring, tail, error  a FRESH unsharded oracle that replays the shard's sub-stream alone (Sub): keyless requests (tatp COMMIT_LOG /
  counts             DELETE_LOG, smallbank COMMIT_LOG) touch only the ring of the shard they are sent to, and a request with a bad
                     type is counted where it arrives."""
from __future__ import annotations

import collections
import functools
from dataclasses import dataclass

import numpy as np

import kvkeys
from dint_amd import wire
from shard_double import fasthash_key, fasthash_lid

W = wire.Workload
KEYLESS = {W.TATP: (int(wire.Tatp.COMMIT_LOG), int(wire.Tatp.DELETE_LOG)), W.SMALLBANK: (int(wire.Sb.COMMIT_LOG),)}
LOCKS = (W.FASST, W.TPL)
_VALID = {W.STORE: (0, 1, 2), W.TATP: (0, 1, 2, 12, 13, 18, 19, 22, 23), W.SMALLBANK: (0, 1, 2, 3, 4, 5, 17)}  # (tatp's COMMIT is no server op)


def n_local(size: int, H: int) -> int:
    return -(-int(size) // H)


def table_sizes(spec, big=False, n_slots=None):
    """the global sizes a home is computed from, for the oracles and engines of tests/opwords.py: [n_slots] / [hash_size] /
    hash_size per table"""
    import opwords as ow

    if spec.wl in LOCKS:
        return [int(ow.N_SLOTS if n_slots is None else n_slots)]
    if spec.wl == W.STORE:
        return [ow.sizes(spec, big)[0] * 18 // 4]
    return list(_kv_sizes(spec.name, big))


@functools.lru_cache(None)
def _kv_sizes(name, big):
    import opwords as ow

    o = ow.oracle(ow.SPECS[name], big)
    return tuple(int(o.hash_size(t)) for t in range(5 if name == "tatp" else 2))


def keyless(wl, req) -> np.ndarray:
    return np.isin(req["type"], KEYLESS[wl]) if wl in KEYLESS else np.zeros(len(req), bool)


def keyed(wl, req) -> np.ndarray:
    """the requests an engine hashes: what a shard that is not their home counts in foreign_requests and echoes (a request with a
    bad type is counted in bad_requests wherever it arrives, a keyless one appends to the ring of whoever gets it)"""
    if wl == W.FASST:
        return req["type"] <= 3
    if wl == W.TPL:
        return ((req["action"] == 0) & (req["type"] <= 1)) | (req["action"] == 1)
    ok = np.isin(req["type"], _VALID[wl])
    return ok & (req["table"] < (5 if wl == W.TATP else 2)) if "table" in req.dtype.names else ok


def global_index(wl, req, sizes) -> np.ndarray:
    """g of every request, from the key or lid it carries (keyless requests carry one too: it decides nothing)"""
    if wl in LOCKS:
        return (fasthash_lid(np.ascontiguousarray(req["lid"], "<u4")) % np.uint64(sizes[0])).astype(np.int64)
    if wl == W.STORE:
        return kvkeys.np_bucket(req["key"], sizes[0]).astype(np.int64)
    hs = np.array(list(sizes) + [1] * 256, np.uint64)[np.minimum(req["table"].astype(np.int64), len(sizes))]
    return (fasthash_key(np.ascontiguousarray(req["key"], "<u8")) % hs).astype(np.int64)


def home(wl, req, sizes, H, rule=0) -> np.ndarray:
    """home rank of every request.  Keyless requests have none and follow `rule`: an int s = all to shard s, "deal" = dealt
    round-robin over the shards in trace order"""
    h = global_index(wl, req, sizes) % H
    kl = keyless(wl, req)
    if kl.any():
        h[kl] = np.arange(int(kl.sum())) % H if rule == "deal" else int(rule)
    return h


# ---- projected state -------------------------------------------------------------------------------------------------------------
def project_rows(dump, hash_size, i, H):
    """the rows of shard i's dump_rows: the oracle's dump is in bucket order with chain order inside a bucket, local = g // H is
    monotone in g, so the filter g % H == i gives the shard's dump, order included"""
    keys, vers, vals = dump
    mine = kvkeys.np_bucket(keys, hash_size).astype(np.int64) % H == i
    return keys[mine], vers[mine], vals[mine]


def _project(a, size, i, H, quadrants):
    nl = n_local(size, H)
    g = np.arange(i, size, H)  # the global indices shard i is home to; local = g // H = 0, 1, 2 ...
    a = np.asarray(a)
    out = np.zeros(quadrants * nl, a.dtype)  # (local slots no global one maps to stay zero)
    for q in range(quadrants):
        out[q * nl:q * nl + len(g)] = a[q * size + g]
    return out


def project_kv_locks(words, hash_size, i, H):
    """oracle word q * hash_size + g -> shard word q * n_local + g // H; the words that correspond to no global bucket (the top
    local bucket where (n_local - 1) * H + i >= hash_size) must be zero"""
    return _project(words, hash_size, i, H, 4)


def project_slots(a, b, n_slots, i, H):
    return _project(a, n_slots, i, H, 1), _project(b, n_slots, i, H, 1)


def projection_index(size, i, H, quadrants=1):
    """for every word of shard i: the oracle word it is projected from, or -1 (the host test's view of the same mapping)"""
    nl = n_local(size, H)
    g = np.arange(nl) * H + i
    one = np.where(g < size, g, -1)
    return np.concatenate([np.where(one >= 0, q * size + one, -1) for q in range(quadrants)])


# ---- a trace on a set ---------------------------------------------------------------------------------------------------------------
@dataclass
class Plan:
    """what every shard of a set is sent: idx[i] = the trace positions in the order sent, own[i] = which of them shard i is home to"""
    H: int
    home: np.ndarray
    idx: dict
    own: dict

    def foreign(self, i):
        return int((~self.own[i]).sum())


def plan(wl, req, hm, H, shards=None, foreign_every=0, also=None):
    """every request to its home, in trace order.  foreign_every = k: shard i receives, besides, every k-th keyed request of the
    other shards, at its place in trace order (they must come back untouched and be counted); also = {rank: mask}: keyed requests
    that this rank is sent besides.  shards: the ranks that exist"""
    shards = list(range(H)) if shards is None else list(shards)
    idx, own = {}, {}
    kd = keyed(wl, req)
    for i in shards:
        take = hm == i
        if foreign_every:
            other = np.nonzero(~take & kd)[0][::foreign_every]
            take = take.copy()
            take[other] = True
        if also is not None and i in also:
            take = take | (also[i] & kd)
        idx[i] = np.nonzero(take)[0]
        own[i] = hm[idx[i]] == i
    return Plan(H, hm, idx, own)


def run_set(engines, req, p: Plan, submit=None):
    """submit every shard what the plan sends it and merge the replies into trace order, each request's from its home shard
    alone.  engines: {rank: engine}; submit(engine, requests) -> replies.  Returns (merged replies, which requests a home answered:
    all of them unless the set lacks ranks); the foreign requests are checked here to have come back byte for byte"""
    submit = submit or (lambda e, r: e.submit(r))
    got = req.copy()
    seen = np.zeros(len(req), bool)
    for i, e in engines.items():
        if not len(p.idx[i]):
            continue
        sent = req[p.idx[i]]
        back = submit(e, sent)
        f = ~p.own[i]
        assert back[f].tobytes() == sent[f].tobytes(), ("a foreign request came back changed from shard", i)
        got[p.idx[i][p.own[i]]] = back[p.own[i]]
        seen[p.idx[i][p.own[i]]] = True
    missing = ~seen & np.isin(p.home, list(engines))
    assert not missing.any(), "a request of an existing shard was sent to nobody"
    return got, seen


# ---- a shard's sub-stream on a fresh oracle: ring, tail and error counts ---------------------------------------------------------------
@dataclass
class Sub:
    replies: list
    tail: int
    ring: np.ndarray   # the records below tail
    errors: int


_SUBS = collections.OrderedDict()


def sub_expected(tag, make_oracle, passes) -> Sub:
    """a fresh unsharded oracle replays `passes` (a shard's own requests, pass by pass); kept per tag, the last 64 (only what is
    compared is kept, not the oracle)"""
    if tag not in _SUBS:
        o = make_oracle()
        rep = [o.replay(p) if len(p) else p.copy() for p in passes]
        tail = int(getattr(o, "tail", 0))
        ring = np.array(o.ring[:tail]) if hasattr(o, "ring") else np.zeros((0, 64), "u1")
        _SUBS[tag] = Sub(rep, tail, ring, int(getattr(o, "errors", 0)))
        while len(_SUBS) > 64:
            _SUBS.popitem(last=False)
    _SUBS.move_to_end(tag)
    return _SUBS[tag]


# ---- fillers by home: dilution of a hot trace with requests of the hot shard or of the others --------------------------------------------
def homed_fillers(spec, n, seed, avoid_key, sizes, H, shard, at_home):
    """n requests as opwords.fillers makes them (they leave every slot and row as it is), all of them with home == shard
    (at_home) or all with another home: sent to `shard`, the latter are foreign requests between the hot ones -- indices without
    a record in the ranges by which a hot key is cut into pieces, holes in the dominant-slot bitmaps"""
    import opwords as ow

    wl = spec.wl
    if wl in LOCKS:
        lids = np.arange(1, 400_001, dtype=np.uint32)
        slot = ow.lid_slot(lids, sizes[0])
        ok = ((slot % H == shard) == at_home) & (slot != ow.lid_slot([avoid_key], sizes[0])[0])
        lids = lids[ok][:64]
        assert len(lids) == 64, len(lids)
        rng = np.random.default_rng(seed)
        if wl == W.FASST:
            return ow.requests(spec, np.zeros(n, np.int64), 0, lids[rng.integers(0, 64, n)], seed)
        j = np.arange(n)
        return ow.requests(spec, np.where(j % 2 == 0, 0x00, 0x10), 0, lids[(j // 2) % 64], seed)
    out, have, k = [], 0, 0
    while have < n:
        f = ow.fillers(spec, 4 * n + 1024, seed + 1000 * k, avoid_key)
        f = f[(home(wl, f, sizes, H) == shard) == at_home]
        out.append(f)
        have += len(f)
        k += 1
        assert k < 64
    return np.concatenate(out)[:n]


def dilute_homed(h, d, sizes, H, shard, at_home):
    """opwords.dilute with homed_fillers: (requests, src)"""
    n = len(h.req)
    out = np.zeros(n + (n - 1) * d, h.req.dtype)
    src = np.full(len(out), -1, np.int64)
    at = np.arange(n) * (d + 1)
    out[at], src[at] = h.req, np.arange(n)
    out[src < 0] = homed_fillers(h.spec, int((src < 0).sum()), 150 + d, h.key, sizes, H, shard, at_home)
    return out, src


# ---- the cases of tests/test_gpu_shard_words.py (tests/test_shardsplit_host.py checks every one of them on the host) --------------------
@dataclass
class SetCase:
    spec: object
    tag: tuple          # names the trace: the unsharded oracle's replay is kept per tag
    H: int
    big: bool
    n_slots: int
    passes: list
    plans: list         # a Plan per pass
    shards: list        # the ranks that are created
    where: object       # where(k, i): names request i of pass k
    hot_shard: int = None

    @property
    def sizes(self):
        return table_sizes(self.spec, self.big, self.n_slots)

    def own(self, i):
        """shard i's own requests, pass by pass: its sub-stream"""
        return [req[p.idx[i][p.own[i]]] for req, p in zip(self.passes, self.plans)]

    def counts(self):
        """{rank: (own keyed requests, own requests, foreign requests)} over all passes"""
        out = {}
        for i in self.shards:
            own = self.own(i)
            out[i] = (sum(int(keyed(self.spec.wl, r).sum()) for r in own), sum(len(r) for r in own), sum(p.foreign(i) for p in self.plans))
        return out


def _case(spec, tag, passes, where, H, *, big=False, n_slots=None, rule=0, shards=None, foreign_every=(), also=(), hot_shard=None):
    """foreign_every / also: per pass (missing: none)"""
    import opwords as ow

    n_slots = ow.N_SLOTS if n_slots is None else n_slots
    sizes = table_sizes(spec, big, n_slots)
    homes = [home(spec.wl, req, sizes, H, rule) for req in passes]
    if shards is None:
        shards = list(range(H))
    elif shards == "receiving":  # the ranks that are home to something, and one more that is sent foreign requests alone
        shards = sorted(set(np.unique(np.concatenate(homes)).tolist()))
        shards += [r for r in ((shards[-1] + 1 + j) % H for j in range(H)) if r not in shards][:1]
    plans = [plan(spec.wl, req, hm, H, shards, foreign_every[k] if k < len(foreign_every) else 0, also[k] if k < len(also) else None)
             for k, (req, hm) in enumerate(zip(passes, homes))]
    return SetCase(spec, tag, H, big, n_slots, passes, plans, list(shards), where, hot_shard)


NEW_LAYOUTS = ("edge", "localline")


def cold_layouts(spec):
    import opwords as ow

    return ow.layouts(spec) + (("localline",) if ow.is_lock(spec) else ("edge",))


@functools.lru_cache(8)
def cold_case(name, target, layout, arr, H) -> SetCase:
    """the preambles in one pass, every request to its home; the words in the next, where every shard is sent every fifth keyed
    request of the others besides.  Keyless requests are dealt round-robin"""
    import opwords as ow

    spec = ow.SPECS[name]
    c = ow.cold_edge(name, H) if layout == "edge" else ow.cold_localline(name, H) if layout == "localline" else ow.cold(name, target, layout)
    req, blk = getattr(c, arr), c.block_of[arr]

    def where(k, i):
        b = int(c.block_of["pre"][i] if k == 0 else blk[i])
        return ("preamble" if k == 0 else "word", b) + c.blocks[b] + (int(c.keys[b]),)

    tag = ("set-cold", name, target, layout, arr) + ((H,) if layout in NEW_LAYOUTS else ())
    return _case(spec, tag, [c.pre, req], where, H, big=layout != "edge", rule="deal", foreign_every=(0, 5))


def hot_shard_of(spec, key, table, sizes, H):
    import opwords as ow

    m = ow.requests(spec, [0], table, key, 0)
    return int(home(spec.wl, m, sizes, H)[0])


SLOT_GEOMETRY = [(1 << 20, 3), (1 << 20, 255), (5, 8), (1, 2)]  # (n_slots, H): 2^20 % 3 = 1, 2^20 % 255 = 16; three shards home to nothing; one slot


@functools.lru_cache(4)
def hot_slot_case(name, n_slots, H, d=0, fill=None, behind=False) -> SetCase:
    """the hot trace on HOT_LID's home.  fill: "home" / "foreign" = d fillers of the hot shard's / of other shards between every two
    hot requests, all sent to the hot shard (the foreign ones to their homes too, where those exist).  behind: 140,000 fillers in
    front, every one to its home.  Every rank is sent every 7th keyed request of the others; with H = 255 there are two ranks, the
    hot one and one that is home to nothing it is sent"""
    import opwords as ow

    spec = ow.SPECS[name]
    h = ow.hot(name, "slot")
    sizes = [n_slots]
    s = hot_shard_of(spec, h.key, 0, sizes, H)
    req, src = (h.req, np.arange(len(h.req))) if not d else dilute_homed(h, d, sizes, H, s, fill == "home")
    n_front = 0
    if behind:
        front = ow.fillers(spec, 140_000, 9, 0)
        req, src, n_front = np.concatenate([front, req]), np.concatenate([np.full(len(front), -1), src]), len(front)

    def where(k, i):
        return ("in front",) if i < n_front else ("filler",) if src[i] < 0 else h.block_at(int(src[i]))

    also = ({s: src < 0},) if fill == "foreign" else ()
    return _case(spec, ("set-hot", name, n_slots, H, d, fill, behind), [req], where, H, n_slots=n_slots,
                 shards=[s, (s + 1) % H] if H > 8 else None, foreign_every=(7,), also=also, hot_shard=s)


@functools.lru_cache(4)
def hot_row_case(name, target, present, H, d=0, rule=None) -> SetCase:
    """the hot trace on the home of its row (smallbank `both`: of its two rows).  d = 0: the ranks that are home to something and
    one more, every rank sent every 7th keyed request of the others.  d > 0: d FOREIGN fillers between every two hot requests,
    sent to the hot shard and to their homes.  Keyless requests go to the hot shard, or (rule "deal") round-robin to all"""
    import opwords as ow

    spec = ow.SPECS[name]
    h = ow.hot(name, target, present)
    sizes = table_sizes(spec)
    s = hot_shard_of(spec, h.key, h.table, sizes, H)
    req, src = (h.req, np.arange(len(h.req))) if not d else dilute_homed(h, d, sizes, H, s, False)

    def where(k, i):
        return ("filler",) if src[i] < 0 else h.block_at(int(src[i]))

    return _case(spec, ("set-hot", name, target, present, H, d, rule), [req], where, H, rule=s if rule is None else rule,
                 shards=None if d or rule == "deal" else "receiving", foreign_every=(7,), also=({s: src < 0},) if d else (), hot_shard=s)


@functools.lru_cache(4)
def dual_case(name, H=3) -> SetCase:
    """two hot traces at once: on two keys of one lock word (so of one shard), on two lids of one LOCAL line of one shard"""
    import opwords as ow

    spec = ow.SPECS[name]
    target = spec.targets[0]
    h = ow.hot(name, target)
    keys = ow.localline_dual_lids(H) if ow.is_lock(spec) else ow.dual_keys(name)
    req, src = ow.dual(name, target, 1, keys=keys)
    s = hot_shard_of(spec, keys[0], h.table, table_sizes(spec), H)
    return _case(spec, ("set-dual", name, H), [req], lambda k, i: ("trace request", int(src[i]), h.block_at(int(src[i]))), H, rule=s,
                 foreign_every=(7,), hot_shard=s)


def _cold_cases():
    import opwords as ow

    out = []
    for name, spec in ow.SPECS.items():
        for k, layout in enumerate(cold_layouts(spec)):
            new = layout in NEW_LAYOUTS
            for j, H in enumerate((2, 3, 8)):
                for arr in ("adjacent", "transposed") if new else (("adjacent", "transposed")[(k + j) % 2],):  # the old layouts: one each
                    for rounds in (False,) if ow.is_lock(spec) else (False, True):
                        out.append((name, spec.targets[0], layout, arr, H, rounds))
    return out


COLD_CASES = _cold_cases()
LOCK_MODES = ("default", "no-direct", "no-fuse", "inputs-ready", "behind-140000")
# (mode, n_slots, H, d, fill)
HOT_SLOT_CASES = ([(m, n, H, 0, None) for n, H in SLOT_GEOMETRY for m in LOCK_MODES if m != "behind-140000" or (n, H) in ((1 << 20, 3), (5, 8))]
                  + [(m, 1 << 20, H, 7, f) for H in (3, 255) for f in ("home", "foreign") for m in ("default", "no-direct")]
                  + [("default", 5, 8, 7, "foreign"), ("ahead-8000", 1 << 20, 3, 0, None)])
ROW_TARGETS = [("tatp", "subscriber", True), ("tatp", "call_forwarding", True), ("store", "row", True), ("smallbank", "saving", True),
               ("smallbank", "both", True)]
# (knob set: an index into SPLIT_KNOBS [0, 2, 3] / SB_KNOBS [0, 1, 5], rounds, max_pass, how): a covering selection of the issue's
# knobs x flags x max_pass, not their product
ROW_MODES = [(0, False, 0, None), (1, False, 0, None), (2, False, 0, None), (1, True, 0, None), (0, False, 5000, None), (1, True, 5000, None)]
# (name, target, present, H, d, mode)
HOT_ROW_CASES = ([(n, t, p, H, 0, m) for n, t, p in ROW_TARGETS for H in (2, 8) for m in ROW_MODES]
                 + [(n, t, p, H, 7, m) for n, t, p in ROW_TARGETS for H in (2, 8) for m in (ROW_MODES[0], ROW_MODES[1])]
                 + [(n, t, False, 8, 0, ROW_MODES[1]) for n, t in (("smallbank", "saving"), ("smallbank", "both"))]
                 + [(n, t, True, 2, 0, (1, False, 0, ("ahead", 8000))) for n, t in (("tatp", "subscriber"), ("store", "row"), ("smallbank", "saving"))])
# the store's hot trace takes two seconds a run (thousands of rows under one key): it keeps every geometry, and of the knobs
# what H = 2 has in pieces, in rounds and across passes, and H = 8 in pieces and in one workgroup
_STORE_KEEP = {(2, 0): (0, 3, 4), (8, 0): (0, 2), (2, 7): (1,), (8, 7): (0,)}
HOT_ROW_CASES = [c for c in HOT_ROW_CASES if c[0] != "store" or c[5][3] or ROW_MODES.index(c[5]) in _STORE_KEEP[c[3], c[4]]]
DUAL_CASES = ["tatp", "smallbank", "lock_fasst", "lock_2pl"]
KEYLESS_CASES = [("tatp", "subscriber"), ("smallbank", "saving")]
SEGMENT_CASES = [(n, kind) for n in ("tatp", "smallbank", "lock_fasst") for kind in ("hot", "cold")]


def segment_case(name, kind, H=3):
    """(the set case, the rank whose home sub-stream goes through submit_segments)"""
    import opwords as ow

    spec = ow.SPECS[name]
    if kind == "cold":
        c = cold_case(name, spec.targets[0], cold_layouts(spec)[-1], "transposed", H)
        return c, max(c.shards, key=lambda i: len(c.own(i)[1]))
    c = hot_slot_case(name, 1 << 20, H) if ow.is_lock(spec) else hot_row_case(name, spec.targets[0], True, H, rule="deal")
    return c, c.hot_shard


def all_trace_cases():
    """every distinct SetCase the GPU tests send, as (id, thunk): what the host test walks"""
    seen = {}
    for name, target, layout, arr, H, _ in COLD_CASES:
        seen[("cold", name, target, layout, arr, H)] = functools.partial(cold_case, name, target, layout, arr, H)
    for name in ("lock_fasst", "lock_2pl"):
        for mode, n, H, d, fill in HOT_SLOT_CASES:
            behind = mode == "behind-140000"
            seen[("slot", name, n, H, d, fill, behind)] = functools.partial(hot_slot_case, name, n, H, d, fill, behind)
    for name, target, present, H, d, _ in HOT_ROW_CASES:
        seen[("row", name, target, present, H, d)] = functools.partial(hot_row_case, name, target, present, H, d)
    for name in DUAL_CASES:
        seen[("dual", name)] = functools.partial(dual_case, name)
    for name, target in KEYLESS_CASES:
        seen[("keyless", name, target)] = functools.partial(hot_row_case, name, target, True, 3, 0, "deal")
    return list(seen.items())
