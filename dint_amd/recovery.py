"""Rebuild a replica from a drained log.

The reference replicates every committed write three ways -- COMMIT_LOG / DELETE_LOG to all three servers, then the
backups, then the primary (tatp/caladan/client_udp_shard.cc:486-570) -- but never reads a log back: there is no
recovery path.  With the log in HBM and `dint_log_drain` streaming it out, recovery is a replay: every
log record becomes the backup operation the client sent right after it (COMMIT_BCK for a row that exists, INSERT_BCK for
one that does not yet, DELETE_BCK for a DELETE_LOG record), in log order, through the ordinary hot path of the
replica being rebuilt.  Because COMMIT_BCK bumps the version and INSERT_BCK starts at 0, a replica that starts from
the same image as the logging server (e.g. the initial population) ends with identical rows AND versions.

Two forms of the same replay.  `apply_log` takes the drained records in host memory and decides in numpy what each
becomes.  `apply_log_device` / `LogShipper` keep the log in HBM from the primary's ring to the replica's tables
(dint_log_drain_device, dint_log_apply_device: csrc/k_replay.hip sorts the records of a chunk by row, probes the replica
once per row and emits the batch on the GPU); primary and replica are engines on the same device, or on peers.

A replica that fell behind (the primary's ring lapped the shipper) cannot be caught up from the log.  `resync` compares the
two engines' tables where they lie (dint_state_diff) and writes the difference into the replica WITH the primary's versions
(dint_state_repair; csrc/k_state.hip); `Engine.state_digest` says in 64 bytes per table whether two engines hold the same rows.
`resync_blocks` is the same for a replica on another device: digests per block of buckets, and only the rows of the blocks that
differ are carried (dint_state_block_digest / _select / _rows / _diff; csrc/k_block.hip).

Moving a server to another shard layout is neither: `reshard` carries the tables of a complete set of engines (1 or G
shards) into a blank set of H shards as state images (dint_state_export / dint_state_import; csrc/k_image.hip) -- entry for
entry, with lock words, duplicate rows, holes and chain order, so that later replies are those of a set sharded that way from
the start.  `save_state` / `load_state` put one engine's own image into a file and back.

An image moves buckets whole, so it cannot change the bucket counts fixed when an engine is created.  `rehash` moves ROWS:
blank engines of another `n_rows` (and, if wanted, another shard count) take the rows of a set of engines where they lie
(dint_state_rehash; csrc/k_rehash.hip) -- every bucket compact, inline entry first, the rows of a bucket in the order the
sources held them, so every key's visible row stays its visible row.  Lock words do not move.

WHEN to do that is what `table_stats` / `rehash_advice` answer: the tables' occupancy and chain shape, computed where they lie
(dint_state_stats; csrc/k_stats.hip), and the small policy on top of it.  `check_tables` lays the chain walk's row count
beside the digest's flat one.

All of it assumes structurally sound tables.  `verify_tables` checks that on a shard set (dint_state_verify;
csrc/k_verify.hip): the census of chains, free lists, pend lists and pool added up, `ok` / `clean`, and on request the leaked
pool entries put back on the free lists.

The lock words are the part of a server's state a crashed client leaves in a bad state: a coordinator that dies between ACQUIRE
and COMMIT / ABORT leaves its locks held for good.  `held_locks` lists what a shard set holds, with global ids (dint_state_locks;
csrc/k_locks_state.hip), and `release_locks` sets the listed units -- or all -- free by compare and release (dint_state_unlock).
"""
from __future__ import annotations

import math

import numpy as np

from ._lib import DintError
from .wire import LOG_REC, SB_MSG, TATP_MSG, Sb, Tatp, Workload


def apply_log(engine, records: np.ndarray) -> dict:
    """records: LOG_REC array as returned by Engine.log_drain / read_log, oldest first."""
    n = len(records)
    if n == 0:
        return {"applied": 0}
    if engine.workload == Workload.SMALLBANK:  # no inserts / deletes: every record is a COMMIT_BCK
        m = np.zeros(n, SB_MSG)
        m["type"], m["table"], m["key"], m["ver"] = Sb.COMMIT_BCK, records["table"], records["key"], records["ver"]
        m["val"] = records["val"][:, :8]
        rep = engine.submit(m)
        return {"applied": n, "acks": int((rep["type"] == Sb.COMMIT_BCK_ACK).sum())}
    assert engine.workload == Workload.TATP
    # which rows exist before the replay: one READ per distinct (table, key)
    tk = (records["table"].astype(np.uint64) << np.uint64(60)) ^ records["key"]  # keys use < 48 bits
    uniq, first, inv = np.unique(tk, return_index=True, return_inverse=True)
    rd = np.zeros(len(uniq), TATP_MSG)
    rd["type"], rd["table"], rd["key"] = Tatp.READ, records["table"][first], records["key"][first]
    exists0 = engine.submit(rd)["type"] == Tatp.GRANT_READ
    # existence before record i = what the previous record on the same row left, else the initial state
    order = np.argsort(inv, kind="stable")
    same_as_prev = np.zeros(n, bool)
    same_as_prev[order[1:]] = inv[order[1:]] == inv[order[:-1]]
    prev = np.empty(n, np.int64)
    prev[order[1:]] = order[:-1]
    prev[order[0]] = order[0]
    is_del = records["is_del"] != 0
    exists = np.where(same_as_prev, ~is_del[prev], exists0[inv])
    m = np.zeros(n, TATP_MSG)
    m["table"], m["key"], m["val"], m["ver"] = records["table"], records["key"], records["val"], records["ver"]
    m["type"] = np.where(is_del, Tatp.DELETE_BCK, np.where(exists, Tatp.COMMIT_BCK, Tatp.INSERT_BCK))
    rep = engine.submit(m)
    return {"applied": n, "commits": int((rep["type"] == Tatp.COMMIT_BCK_ACK).sum()),
            "inserts": int((rep["type"] == Tatp.INSERT_BCK_ACK).sum()), "deletes": int((rep["type"] == Tatp.DELETE_BCK_ACK).sum())}


def apply_log_device(engine, d_records, n: int, chunk: int = 0) -> dict:
    """apply_log for records that live in HBM (a torch uint8 tensor or a device pointer; n 64-byte records, oldest
    first, e.g. filled by Engine.log_drain_device): same result, same keys.  `chunk` = records per pass, 0 = pass_max."""
    if n == 0:
        return {"applied": 0}
    st = engine.log_apply_device(d_records, n, chunk)
    if engine.workload == Workload.SMALLBANK:
        return {"applied": n, "acks": st["commits"]}
    return {"applied": n, "commits": st["commits"], "inserts": st["inserts"], "deletes": st["deletes"]}


def apply_log_folded(engine, d_records, n: int, chunk: int = 0) -> dict:
    """apply_log_device through the fold (Engine.log_apply_folded; csrc/k_fold.hip, csrc/log_fold.h): the same rows afterwards,
    the same keys with the same counts, plus `folded` and `deferred` -- the records whose row's net effect the state repair wrote,
    and the ones that went through the serial replay."""
    if n == 0:
        return {"applied": 0}
    st = engine.log_apply_folded(d_records, n, chunk)
    if engine.workload == Workload.SMALLBANK:
        out = {"applied": n, "acks": st["commits"]}
    else:
        out = {"applied": n, "commits": st["commits"], "inserts": st["inserts"], "deletes": st["deletes"]}
    out["folded"], out["deferred"] = st["folded_records"], st["deferred_records"]
    return out


def fold_log_host(workload, hash_size, dumps, records) -> tuple:
    """dint_log_fold_host (include/dint_driver.h): ONE chunk of records folded on the host against dumped rows.  dumps[t] = (keys,
    vers, ...) of table t as Engine.dump_rows returns them; hash_size[t] = the table's bucket count.  Returns
    (deferred flags per record, repair records as a LOG_REC array, stats).  No device call."""
    import ctypes as C

    from . import _lib

    records = np.ascontiguousarray(records)
    nt = len(dumps)
    off = np.zeros(nt + 1, "<u8")
    off[1:] = np.cumsum([len(d[0]) for d in dumps])
    keys = np.ascontiguousarray(np.concatenate([np.asarray(d[0], "<u8") for d in dumps]), "<u8")
    vers = np.ascontiguousarray(np.concatenate([np.asarray(d[1], "<u4") for d in dumps]), "<u4")
    hs = np.ascontiguousarray(hash_size, "<u8")
    n = len(records)
    deferred = np.zeros(max(n, 1), np.uint8)
    repair = np.zeros(max(n, 1), LOG_REC)
    s = _lib.FoldStats()
    got = _lib.check(_lib.load().dint_log_fold_host(int(workload), nt, hs.ctypes.data, off.ctypes.data, keys.ctypes.data, vers.ctypes.data,
                                                    records.ctypes.data, n, deferred.ctypes.data, repair.ctypes.data, n, C.byref(s)))
    return deferred[:n].astype(bool), repair[:got], s.as_dict()


def digests_equal(a, b) -> bool:
    """do the two engines hold the same rows (keys, versions, values), whatever their chains look like?"""
    return a.state_digest() == b.state_digest()


def resync(primary, replica, cap: int = 1 << 20, max_rounds: int = 8, buf=None) -> dict:
    """Make the replica's rows equal the primary's without leaving the GPU: rounds of state_diff -> state_repair through one
    HBM buffer of `cap` records until the diff is empty.  Several rounds when the diff is longer than `cap`, or when the
    replica holds duplicate rows of a key (the diff sees the visible row only; deleting it uncovers the next).  Returns
    {rounds: repair calls made, records: records applied, digests_equal}.  What the diff cannot see is not repaired -- a
    shadowed duplicate of a key that stays visible, on either side -- and digests_equal, the strict check, then says False
    (as it does when max_rounds did not suffice).  The caller keeps both engines quiet for the
    duration; both must be engines of one workload and size on one device: unsharded, or the SAME shard of two sets, every sharded
    one created with FLAG_SHARD_REPLICA (the diff is then in that shard's local bucket order, which its repair takes)."""
    import torch

    if buf is None:
        buf = torch.empty(cap * LOG_REC.itemsize, dtype=torch.uint8, device="cuda")
    rounds = records = 0
    while True:
        n, st = primary.state_diff(replica, buf, cap)
        if st["total"] == 0 or rounds >= max_rounds:
            break
        records += replica.state_repair(buf, n)["applied"]
        rounds += 1
    return {"rounds": rounds, "records": records, "digests_equal": digests_equal(primary, replica)}


def resync_blocks(primary, replica, block_buckets: int = 4096, cap: int = 1 << 20, max_rounds: int = 8, carry=None) -> dict:
    """`resync` for a replica on ANOTHER device: the two sides compare digests of blocks of `block_buckets` buckets
    (Engine.state_block_digest; csrc/state_block.h) and only the rows of the blocks that differ travel.  A round: block digests on
    both sides; the primary's carried over; select on the replica; the differing ids carried back; their visible rows on the
    primary (state_block_rows); the rows carried over; state_block_diff then state_repair on the replica.  `carry(tensor)` moves
    a tensor from one engine's device to the other's -- default: `.to()` the other engine's device; everything else stays where
    it is.  Rounds repeat as `resync`'s do: a deleted visible duplicate uncovers the next, and `cap` (records per buffer, one
    on each side) may be shorter than the rows or the diff -- then a round takes the leading blocks whose rows fit, so one block's
    rows must fit `cap`.  Returns {rounds, records, blocks_differing (in the first round), digest_bytes, id_bytes, row_bytes
    (what was carried), digests_equal (Engine.state_digest, the strict check)}.  Equal replicas cost the two digest calls and one
    select and carry the digests only.  Both engines: one workload, n_rows and flags, quiet for the duration; unsharded, or
    the same shard of two sets with the replica created with FLAG_SHARD_REPLICA (the block calls take any shard; the repair that
    applies their result takes a flagged one)."""
    import torch

    to_replica = carry if carry is not None else (lambda t: t.to(replica._torch_device()))
    to_primary = carry if carry is not None else (lambda t: t.to(primary._torch_device()))
    out = {"rounds": 0, "records": 0, "blocks_differing": 0, "digest_bytes": 0, "id_bytes": 0, "row_bytes": 0}
    rows_buf = rec_buf = None
    while True:
        da, nb, _ = primary.state_block_digest(block_buckets)
        db, nb_r, _ = replica.state_block_digest(block_buckets)
        if nb != nb_r:
            raise DintError(f"resync_blocks: {nb} blocks on the primary, {nb_r} on the replica: not engines of one size and shard")
        da_r = to_replica(da[:nb])
        out["digest_bytes"] += 32 * nb
        ids, nd = replica.state_block_select(da_r, db, nb)
        if out["rounds"] == 0:
            out["blocks_differing"] = nd
        if nd == 0 or out["rounds"] >= max_rounds:
            break
        ids_p = to_primary(ids[:nd])
        out["id_bytes"] += 4 * nd
        take = nd
        while True:  # the leading blocks whose rows fit the buffer
            _, total = primary.state_block_rows(block_buckets, ids_p, take)
            if total <= cap:
                break
            if take == 1:
                raise DintError(f"resync_blocks: block {int(ids[0])} holds {total} rows, the buffers {cap}: a larger cap or smaller blocks")
            take //= 2
        if rows_buf is None:
            rows_buf = torch.empty(cap * LOG_REC.itemsize, dtype=torch.uint8, device=primary._torch_device())
            rec_buf = torch.empty(cap * LOG_REC.itemsize, dtype=torch.uint8, device=replica._torch_device())
        n, _ = primary.state_block_rows(block_buckets, ids_p, take, rows_buf, cap)
        rows_r = to_replica(rows_buf[:n * LOG_REC.itemsize])
        out["row_bytes"] += n * LOG_REC.itemsize
        m, st = replica.state_block_diff(block_buckets, ids, take, rows_r, n, rec_buf, cap)
        if m:
            out["records"] += replica.state_repair(rec_buf, m)["applied"]
        out["rounds"] += 1
        if st["total"] == 0 and take == nd:
            break  # (the blocks differ in what the diff does not see: shadowed duplicates; digests_equal says so)
    out["digests_equal"] = digests_equal(primary, replica)
    return out


def route_records(geom, d_records, n: int, dst_count: int, d_out=None, stream: int = 0) -> list:
    """Engine.records_route as views: the n records at d_records (a torch uint8 tensor in HBM) routed to a layout of `dst_count`
    shards; returns [(tensor view of shard h's records, their number) for h in range(dst_count)] -- pieces of ONE buffer, each in
    the input's order.  `geom` = any engine of the workload and n_rows on that device (its own shard layout does not matter)."""
    out, off = geom.records_route(dst_count, d_records, n, d_out, stream)
    return [(out[64 * off[h]:64 * off[h + 1]], off[h + 1] - off[h]) for h in range(dst_count)]


def _layout(engines) -> int:
    engines = list(engines)
    G = len(engines)
    if not all(e.shard_count == G and e.shard_index == i for i, e in enumerate(engines)):
        raise DintError("a shard set is a complete layout in index order: shard i of G at position i")
    return G


def resync_set(primaries, replicas, blocks=None, carry=None, cap: int = 1 << 20) -> dict:
    """`resync` (blocks=None) or `resync_blocks` (blocks=B buckets per block; `carry` as there) pair by pair for two shard sets of
    ONE layout: replica shard i := primary shard i.  The replicas carry FLAG_SHARD_REPLICA, and for blocks=None so do the
    primaries (state_diff compares flagged shards only; the block calls take any shard).  One engine on each side: plain `resync`.  Returns {"shards": the per-pair results, "records": their sum, "digests_equal": digest_sum of the two sets is
    equal}.  Sets of different layouts are refused: moving tables between layouts is `reshard`'s job (state images), not a
    resync's."""
    primaries, replicas = list(primaries), list(replicas)
    G, H = _layout(primaries), _layout(replicas)
    if G != H:
        raise DintError(f"resync_set: {G} primary shards, {H} replica shards: a resync pairs equal layouts; recovery.reshard moves "
                        "tables to another layout")
    per = [resync(p, r, cap=cap) if blocks is None else resync_blocks(p, r, block_buckets=blocks, cap=cap, carry=carry)
           for p, r in zip(primaries, replicas)]
    return {"shards": per, "records": sum(x["records"] for x in per), "digests_equal": digest_sum(primaries) == digest_sum(replicas)}


def image_pieces(G: int, H: int) -> list:
    """the (i, j) for which the image of source shard i of G for destination shard j of H can hold anything: a global bucket g
    with g % G == i and g % H == j exists iff i == j mod gcd(G, H)"""
    G, H = max(1, G), max(1, H)
    d = math.gcd(G, H)
    return [(i, j) for i in range(G) for j in range(H) if i % d == j % d]


def _image_check_host(image: np.ndarray) -> None:
    from . import _lib

    image = np.ascontiguousarray(image, np.uint8)
    _lib.check(_lib.load().dint_state_image_check_host(image.ctypes.data, image.nbytes))


def reshard(src_engines, dst_engines, buf=None) -> dict:
    """Move the tables of `src_engines` (a complete layout: shard i of G at position i) into `dst_engines` (shard j of H at
    position j), all on one device: every compatible piece (image_pieces) is exported into one HBM buffer and imported from
    it.  Resets nothing: the destinations must be blank (created or reset, nothing but imports since).  The sources are left
    untouched; their log rings are not moved (drain them first).  `buf` = a torch uint8 tensor to use (grown when a piece
    is larger).  Returns the summed stats {bytes, buckets, overflow_entries, rows, pieces}."""
    G, H = len(src_engines), len(dst_engines)
    assert all(e.shard_count == G and e.shard_index == i for i, e in enumerate(src_engines)), "sources: a complete layout in index order"
    assert all(e.shard_count == H and e.shard_index == j for j, e in enumerate(dst_engines)), "destinations: a complete layout in index order"
    tot = {"bytes": 0, "buckets": 0, "overflow_entries": 0, "rows": 0, "pieces": 0}
    for i, j in image_pieces(G, H):
        if buf is None:
            buf, n, _ = src_engines[i].state_export(j, H)
        else:
            try:
                _, n, _ = src_engines[i].state_export(j, H, buf)
            except DintError:
                if src_engines[i].last_image["bytes"] <= buf.numel():
                    raise
                buf, n, _ = src_engines[i].state_export(j, H)  # (too small: a buffer of the piece's size from here on)
        st = dst_engines[j].state_import(buf, n)
        for k in ("bytes", "buckets", "overflow_entries", "rows"):
            tot[k] += st[k]
        tot["pieces"] += 1
    return tot


def rehash(src_engines, dst_engines, drop_locks: bool = False) -> dict:
    """Move the rows of `src_engines` into `dst_engines` -- BLANK engines of the same workload and flags on the same device,
    with their own n_rows, pool_entries and shard layout: every destination takes all sources (Engine.state_rehash) and keeps
    the rows that are home to it.  With a complete destination set (shard j of H at position j) every row lands exactly once;
    this is checked -- the placed rows sum to the sources' rows and the summed digests are equal -- and DintError is raised
    otherwise.  Sources that hold lock words are refused unless drop_locks (a lock word belongs to a slot of the old size);
    `held_locks(src_engines)` shows which units a refusal is about -- slot, counters, owner or candidate key -- and
    `release_locks(src_engines, records)` sets the orphaned ones free, after which the rehash goes through without dropping any.
    The sources are only read; their log rings are not moved (drain them first).  Returns {rows_seen, rows_placed,
    locks_held, tables: per table {rows, overflow_entries, longest_chain} over the destinations, per_engine: [stats]}.

    Growing one server in place::

        big = Engine(Workload.TATP, n_rows=2 * n, pool_entries=..., log_entries=...)   # blank
        recovery.rehash([server], [big])       # server is quiet meanwhile; a DintError leaves `big` blank and says what it takes
        server, old = big, server              # swap: later requests go to `big`
        old.close()
    """
    src_engines, dst_engines = list(src_engines), list(dst_engines)
    per = [d.state_rehash(src_engines, drop_locks=drop_locks) for d in dst_engines]
    tot = {"rows_seen": per[0]["rows_seen"] if per else 0, "rows_placed": sum(p["rows_placed"] for p in per),
           "locks_held": per[0]["locks_held"] if per else 0, "per_engine": per, "tables": []}
    for t in range(len(per[0]["tables"]) if per else 0):
        tot["tables"].append({"rows": sum(p["tables"][t]["rows"] for p in per),
                              "overflow_entries": sum(p["tables"][t]["overflow_entries"] for p in per),
                              "longest_chain": max(p["tables"][t]["longest_chain"] for p in per)})
    if tot["rows_placed"] != tot["rows_seen"]:
        raise DintError(f"rehash: the destinations placed {tot['rows_placed']} of the sources' {tot['rows_seen']} rows: not a complete shard set")
    if digest_sum(src_engines) != digest_sum(dst_engines):
        raise DintError("rehash: the destinations' digests do not add up to the sources'")
    return tot


#: a row of held_locks: dint_lock_record's fields plus where the unit lives in the set and its GLOBAL ids
HELD_LOCK = np.dtype([("shard", "<u4"), ("slot", "<u8"), ("a", "<u4"), ("b", "<u4"), ("key", "<u8"), ("cand_rows", "<u4"), ("table", "u1"),
                      ("flags", "u1"), ("q", "u1"), ("bucket", "<u8"), ("lock_hash", "<u8")])


def held_locks(engines) -> np.ndarray:
    """The lock units a set of engines holds (Engine.state_locks per engine), merged into one numpy array of HELD_LOCK in set
    order: `shard` = the engine's position, slot / a / b / key / cand_rows / table / flags as the engine reported them, and the
    GLOBAL ids added.  Lock tables: bucket = lock_hash = the global slot, local * H + index.  tatp / smallbank: q = the unit's
    quadrant, bucket = the global bucket local * H + index, lock_hash = q * hash_size + bucket -- what fasthash64(key) %
    (4 * hash_size) of every key that can hold the unit is.  H and index are each engine's own shard_count and shard_index."""
    from .engine import lock_records

    out = []
    for pos, e in enumerate(engines):
        buf, n, _ = e.state_locks()
        r = lock_records(buf, n)
        h = np.zeros(n, HELD_LOCK)
        for k in ("slot", "a", "b", "key", "cand_rows", "table", "flags"):
            h[k] = r[k]
        h["shard"] = pos
        H, i = np.uint64(e.shard_count), np.uint64(e.shard_index)
        if e.workload in (Workload.TATP, Workload.SMALLBANK):
            hs = np.array([e.hash_size(int(t)) for t in r["table"]], np.uint64)
            n_local = (hs + H - np.uint64(1)) // H
            q = r["slot"] // np.maximum(n_local, np.uint64(1))
            h["q"] = q
            h["bucket"] = (r["slot"] - q * n_local) * H + i
            h["lock_hash"] = q * hs + h["bucket"]
        else:
            h["bucket"] = h["lock_hash"] = r["slot"] * H + i
        out.append(h)
    return np.concatenate(out) if out else np.zeros(0, HELD_LOCK)


def release_locks(engines, records=None, dry_run: bool = False) -> dict:
    """Release lock units of a set of engines.  records=None: every held unit of every engine (Engine.state_unlock(all=True)).
    Otherwise `records` = rows of held_locks over THIS set, in any selection that keeps each shard's rows in their order: per
    shard they are uploaded and released by compare and release, so a unit that was released and taken again since the listing
    is left alone and counted "stale".  dry_run=True only counts.  Returns {released, stale, released_a, released_b,
    per_table, per_engine: [Engine.state_unlock's dict]}; a shard's list that is refused raises DintError, nothing of THAT
    shard released."""
    import torch

    from .engine import LOCK_REC

    engines = list(engines)
    per = []
    for pos, e in enumerate(engines):
        if records is None:
            per.append(e.state_unlock(all=True, dry_run=dry_run))
            continue
        mine = records[records["shard"] == pos]
        rec = np.zeros(len(mine), LOCK_REC)
        for k in ("slot", "a", "b", "key", "cand_rows", "table", "flags"):
            rec[k] = mine[k]
        if len(rec) == 0:
            per.append(e.state_unlock(None, 0, dry_run=dry_run))
            continue
        d = torch.from_numpy(rec.view(np.uint8).copy()).to(e._torch_device())
        per.append(e.state_unlock(d, len(rec), dry_run=dry_run))
    tot = {k: sum(p[k] for p in per) for k in ("released", "stale", "released_a", "released_b")}
    tot["per_table"] = [sum(p["per_table"][t] for p in per) for t in range(5)]
    tot["per_engine"] = per
    return tot


def populate_set(engines, n: int) -> dict:
    """The reference's population of the first n subscribers / accounts into a shard set of BLANK engines without the host
    (Engine.populate_device): every engine generates all rows on its device and keeps the ones that are home to it.  With a
    complete set (shard j of H at position j) every row lands exactly once; this is checked -- each row is loaded by one engine
    and foreign to the H - 1 others -- and DintError is raised otherwise.  Returns {rows_loaded, temp_bytes: the largest peak,
    tables: per table {rows, overflow_entries, longest_chain_entries} over the set, per_engine: [Engine.last_load]}."""
    engines = list(engines)
    per = [e.populate_device(n) for e in engines]
    tot = {"rows_loaded": sum(p["rows_loaded"] for p in per), "temp_bytes": max([p["temp_bytes"] for p in per] or [0]),
           "per_engine": per, "tables": []}
    for t in range(len(per[0]["tables"]) if per else 0):
        tot["tables"].append({"rows": sum(p["tables"][t]["rows"] for p in per),
                              "overflow_entries": sum(p["tables"][t]["overflow_entries"] for p in per),
                              "longest_chain_entries": max(p["tables"][t]["longest_chain_entries"] for p in per)})
    if per and sum(p["foreign_rows"] for p in per) != (len(per) - 1) * tot["rows_loaded"]:
        raise DintError(f"populate_set: {tot['rows_loaded']} rows loaded by {len(per)} engines, {sum(p['foreign_rows'] for p in per)} "
                        "found foreign: not a complete shard set")
    return tot


def digest_sum(engines) -> list:
    """the digests of a set of engines added up per table: rows and sum add, xr xors (Engine.state_digest)"""
    out = None
    for e in engines:
        d = e.state_digest()
        if out is None:
            out = [dict(x) for x in d]
        else:
            for x, y in zip(out, d):
                x["rows"] += y["rows"]; x["sum"] = (x["sum"] + y["sum"]) % (1 << 64); x["xr"] ^= y["xr"]
    return out


_SUMMED = ("buckets", "buckets_empty", "rows", "entries", "overflow_entries", "holes", "inline_first", "inline_unlinked", "hit_entries",
           "shadowed_rows", "buckets_unchecked", "locks_held", "pool_cap", "pool_top")
NO_BUCKET = (1 << 64) - 1  #: longest_chain_bucket of a table without rows


def merge_table_stats(reports) -> list:
    """per-table reports of several engines (Engine.state_stats) as one: counters and histograms add, longest_chain and most_rows
    take the maximum, longest_chain_bucket goes with the longest chain (ties: the lowest global id)"""
    out = None
    for rep in reports:
        if out is None:
            out = [dict(x, chain_hist=list(x["chain_hist"]), rows_hist=list(x["rows_hist"])) for x in rep]
            continue
        for x, y in zip(out, rep):
            for k in _SUMMED:
                x[k] += y[k]
            for k in ("chain_hist", "rows_hist"):
                x[k] = [p + q for p, q in zip(x[k], y[k])]
            if (y["longest_chain"], -y["longest_chain_bucket"]) > (x["longest_chain"], -x["longest_chain_bucket"]):
                x["longest_chain"], x["longest_chain_bucket"] = y["longest_chain"], y["longest_chain_bucket"]
            x["most_rows"] = max(x["most_rows"], y["most_rows"])
    return out or []


def table_stats(engines) -> list:
    """Engine.state_stats of a sharded set (or any set of engines of one workload) summed per table: see merge_table_stats.
    pool_cap and pool_top add as well."""
    return merge_table_stats(e.state_stats() for e in engines)


def check_tables(engine) -> dict:
    """The valid-slot invariant on a live engine: Engine.state_digest is a FLAT scan, right only while a valid byte is set
    nowhere but in an entry linked into its bucket's chain; Engine.state_stats counts the valid slots a CHAIN WALK reaches.  The
    two row counts taken back to back: {"ok": equal for every table, "tables": the report per table with "digest_rows" beside
    "rows"}.  Two existing numbers compared; the engine is quiet meanwhile."""
    st, dg = engine.state_stats(), engine.state_digest()
    tables = [dict(s, digest_rows=d["rows"]) for s, d in zip(st, dg)]
    return {"ok": all(t["rows"] == t["digest_rows"] for t in tables), "tables": tables}


#: the counts of a verify report that say "this table is damaged" (Engine.state_verify; csrc/state_verify.h)
VERIFY_VIOLATIONS = ("bad_chains", "cross_linked", "linked_beyond_top", "list_bad_links", "stray_valid_entries", "stray_rows",
                     "misplaced_rows", "odd_valid_bytes")


def verify_tables(engines, reclaim: bool = False) -> dict:
    """Engine.state_verify (reclaim=True: Engine.state_reclaim) of every engine of a set -- a shard set, or any engines of one
    workload -- and the reports added up per table: every count adds, longest_list takes the maximum.  Returns {"ok": every
    violation count of every table is 0, "clean": ok and nothing unaccounted (before a reclaim: the census is taken first),
    "tables": the sums per table, "engines": the reports per engine}.  A refused reclaim raises DintError like the engine call."""
    per = [e.state_reclaim() if reclaim else e.state_verify() for e in engines]
    tables = None
    for rep in per:
        if tables is None:
            tables = [dict(x) for x in rep]
            continue
        for x, y in zip(tables, rep):
            for k in x:
                x[k] = max(x[k], y[k]) if k == "longest_list" else x[k] + y[k]
    tables = tables or []
    ok = all(t[k] == 0 for t in tables for k in VERIFY_VIOLATIONS)
    return {"ok": ok, "clean": ok and all(t["unaccounted"] == 0 for t in tables), "tables": tables, "engines": per}


def hash_sizes(workload, n_rows: int) -> list:
    """the global bucket count of every table of an engine created with n_rows: dint_kv_create's formulas (csrc/dint_kv.h dint_kv_hash_sizes),
    mirrored -- what Engine.hash_size(t) returns.  n_rows = 0 is the reference's own size."""
    wl = Workload(workload)
    if wl == Workload.STORE:
        n = n_rows or 2_000_000
        hs = [n * 18 // 4]
    elif wl == Workload.TATP:
        n = n_rows or 7_000_000
        hs = [n * 3 // 2 // 4] * 2 + [n * 15 // 4 // 4] * 2 + [n * 45 // 8 // 4]
    elif wl == Workload.SMALLBANK:
        n = n_rows or 24_000_000
        hs = [n * 3 // 2 // 4] * 2
    else:
        raise ValueError(f"{wl!r} has no kv table")
    return [max(1, h) for h in hs]


def advise_n_rows(workload, rows, rows_per_bucket=8 / 3) -> int:
    """the smallest n_rows >= 1 for which every table t has at least rows[t] / rows_per_bucket buckets (hash_sizes)"""
    from fractions import Fraction

    rpb = Fraction(rows_per_bucket).limit_denominator(1 << 20)
    need = [math.ceil(Fraction(int(r)) / rpb) for r in rows]

    def fits(n):
        return all(h >= w for h, w in zip(hash_sizes(workload, n), need))

    hi = 1
    while not fits(hi):
        hi *= 2
    lo = hi // 2  # (lo does not fit, or is 0; the bucket counts never fall as n_rows grows)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if fits(mid) else (mid, hi)
    return hi


def rehash_advice(engines, rows_per_bucket=8 / 3, max_rows_per_bucket=4.0, max_pool_fill=0.5) -> dict:
    """Is it time to rehash this set of engines (a complete shard set, or one engine), and to which n_rows?  Policy only: one
    Engine.state_stats per engine, no other device work.

    load of table t = its rows over the set / its GLOBAL bucket count.  `needed` is true when any table's load exceeds
    max_rows_per_bucket, or any table of any engine has more than max_pool_fill of its overflow pool linked
    (overflow_entries / pool_cap).  `n_rows` is the smallest value for which every table gets at least rows / rows_per_bucket
    buckets (advise_n_rows) -- what to create the destinations of `rehash` with, needed or not.  `locks_held` non-zero says
    `rehash` will need drop_locks=True.  The destination's pool stays with the existing mechanism: a DintError (DINT_ENOMEM)
    of `rehash` reports the need per table.

    The thresholds are ARGUMENTS, not tuned numbers: 8/3 is the reference's own load (12 rows x 3/2 / 4 slots, the lines
    dint_kv_create cites), 4.0 the capacity of the inline entry -- beyond it the average bucket overflows -- and 0.5 leaves
    half the pool for the churn to come.  Returns {needed, n_rows, load: [per table], pool_fill: the largest, locks_held,
    tables: table_stats}."""
    engines = list(engines)
    per = [e.state_stats() for e in engines]
    tables = merge_table_stats(per)
    load = [t["rows"] / engines[0].hash_size(k) for k, t in enumerate(tables)]
    pool_fill = max((t["overflow_entries"] / t["pool_cap"] for rep in per for t in rep if t["pool_cap"]), default=0.0)
    return {"needed": any(x > max_rows_per_bucket for x in load) or pool_fill > max_pool_fill,
            "n_rows": advise_n_rows(engines[0].workload, [t["rows"] for t in tables], rows_per_bucket),
            "load": load, "pool_fill": pool_fill, "locks_held": sum(t["locks_held"] for t in tables), "tables": tables}


def compact_tables(engines, dry_run: bool = False) -> dict:
    """Engine.state_compact of every engine of a set -- a shard set, or any engines of one workload -- and the reports added up
    per table, as verify_tables does for the census: every count adds ("verify": as verify_tables adds it).  Returns {"tables":
    the sums per table, "engines": the reports per engine}.  A refused compaction raises DintError like the engine call; the
    engines before it are compacted then (dry_run=True first, to ask every engine before any is touched)."""
    per = [e.state_compact(dry_run=dry_run) for e in engines]
    tables = None
    for rep in per:
        if tables is None:
            tables = [dict(x, verify=dict(x["verify"])) for x in rep]
            continue
        for x, y in zip(tables, rep):
            for k in x:
                if k != "verify":
                    x[k] += y[k]
            for k in x["verify"]:
                x["verify"][k] = max(x["verify"][k], y["verify"][k]) if k == "longest_list" else x["verify"][k] + y["verify"][k]
    return {"tables": tables or [], "engines": per}


def compact_advice(engines, rows_per_bucket=8 / 3, max_rows_per_bucket=4.0, max_pool_fill=0.5, max_hole_share=0.25,
                   max_pool_top_fill=0.75) -> dict:
    """Compact this set of engines in place, rehash it, or leave it?  Policy only: one Engine.state_stats and one dry run of
    Engine.state_compact per engine, nothing written.  rehash_advice is not changed by this and still answers its own question.

    "rehash"   the bucket count itself is too small: a table's load (rows over the set / GLOBAL bucket count) exceeds
               max_rows_per_bucket, or some table of some engine would still have more than max_pool_fill of its pool linked
               AFTER a compaction (overflow_after / pool_cap) -- its chains need more buckets, not a tidier layout
    "compact"  otherwise, when the layout has decayed: hole_share -- the slots a compaction gives back, (holes_before -
               holes_after) / (4 * entries_before), the largest over tables and engines -- exceeds max_hole_share, or
               pool_top_fill -- min(pool_top, pool_cap) / pool_cap, the largest -- exceeds max_pool_top_fill
    "none"     otherwise

    The thresholds are ARGUMENTS, not tuned numbers: the first three are rehash_advice's; 0.25 says a quarter of the slots a
    lookup walks past are dead weight, one header sector in four; 0.75 leaves a quarter of the pool to the bump allocator
    before every inserting run of a pass goes request by request.  Returns {action, n_rows (rehash_advice's: what to create
    the destinations of a rehash with), load, hole_share, pool_top_fill, pool_top_fill_after, locks_held (a rehash needs
    drop_locks=True then; a compaction does not care), tables: table_stats, compact: compact_tables' sums}."""
    engines = list(engines)
    per = [e.state_stats() for e in engines]
    dry = compact_tables(engines, dry_run=True)
    tables = merge_table_stats(per)
    load = [t["rows"] / engines[0].hash_size(k) for k, t in enumerate(tables)]
    each = [(c, s["pool_cap"]) for rep, srep in zip(dry["engines"], per) for c, s in zip(rep, srep)]
    hole_share = max(((c["holes_before"] - c["holes_after"]) / (4 * c["entries_before"]) for c, _ in each if c["entries_before"]), default=0.0)
    top_fill = max((min(c["pool_top_before"], cap) / cap for c, cap in each if cap), default=0.0)
    fill_after = max((c["overflow_after"] / cap for c, cap in each if cap), default=0.0)
    if any(x > max_rows_per_bucket for x in load) or fill_after > max_pool_fill:
        action = "rehash"
    elif hole_share > max_hole_share or top_fill > max_pool_top_fill:
        action = "compact"
    else:
        action = "none"
    return {"action": action, "n_rows": advise_n_rows(engines[0].workload, [t["rows"] for t in tables], rows_per_bucket),
            "load": load, "hole_share": hole_share, "pool_top_fill": top_fill, "pool_top_fill_after": fill_after,
            "locks_held": sum(t["locks_held"] for t in tables), "tables": tables, "compact": dry["tables"]}


def save_state(engine, path) -> dict:
    """The engine's own image -- (i, G) -> (i, G): tables, chains and lock words -- written to a file.  The log ring is NOT
    part of it (nor are the pool's free lists): drain the log first if its records matter."""
    buf, n, st = engine.state_export(engine.shard_index, engine.shard_count)
    buf[:n].cpu().numpy().tofile(path)
    return st


def load_state(engine, path) -> dict:
    """A file written by save_state into a BLANK engine of the same workload, size, flags and shard.  The file is checked on
    the host first (dint_state_image_check_host), then uploaded and checked again where it lies.  The log ring is not part
    of a saved state: the engine's stays as it was."""
    import torch

    image = np.fromfile(path, np.uint8)
    _image_check_host(image)
    buf = torch.from_numpy(image).to("cuda")
    return engine.state_import(buf, image.nbytes)


class LogShipper:
    """Follows a primary's log into a replica: `step()` drains what the primary appended since the last step into one
    HBM buffer of `cap` records and replays it.  The records never reach host memory (the drain reads the ring's 16-byte
    tail words, nothing else).  Step at least once per `primary` log ring of appends, or `lost` says what the ring
    overwrote; a step takes at most `cap` records, the rest waits for the next one.

    What the ring overwrote cannot be replayed: `resync()` brings the replica back from the primary's tables instead, and
    with resync_on_loss=True `step()` does so by itself when it finds records lost.  The caller keeps both engines quiet
    for the duration of a resync (no submissions to either)."""

    def __init__(self, primary, replica, cap: int = 1 << 20, chunk: int = 0, resync_on_loss: bool = False, fold: bool = False):
        import torch

        assert primary.workload == replica.workload
        self.primary, self.replica, self.cap, self.chunk = primary, replica, cap, chunk
        self.buf = torch.empty(cap * LOG_REC.itemsize, dtype=torch.uint8, device="cuda")
        self.shipped = self.lost = self.resyncs = 0
        self.resync_on_loss = resync_on_loss
        self.fold = fold  # replay through apply_log_folded: step() then adds `folded` and `deferred`

    def step(self) -> dict:
        n, lost = self.primary.log_drain_device(self.buf, self.cap)
        if lost and self.resync_on_loss:
            # the drained records are part of what the primary's tables already hold: dropped, not replayed
            self.lost += lost
            return {"applied": 0, "lost": lost, "resync": self.resync()}
        out = (apply_log_folded if self.fold else apply_log_device)(self.replica, self.buf, n, self.chunk)
        out["lost"] = lost
        self.shipped += n
        self.lost += lost
        return out

    def resync(self, blocks=None) -> dict:
        """Replica := primary, from the tables.  First the primary's drain cursor moves to the tail (a drain whose records
        are dropped): the records still in the ring are in the primary's rows already, and replayed on top of the repaired
        replica they would bump versions twice.  Both engines quiet for the duration.  blocks=B: through `resync_blocks` with
        blocks of B buckets (a replica on another device); None: `resync`."""
        while True:
            n, _ = self.primary.log_drain_device(self.buf, self.cap)
            if n == 0:
                break
        if blocks is None:
            out = resync(self.primary, self.replica, cap=self.cap, buf=self.buf)
        else:
            out = resync_blocks(self.primary, self.replica, block_buckets=blocks, cap=self.cap)
        self.resyncs += 1
        return out


class ShardSetShipper:
    """`LogShipper.step()` for shard SETS: follows the logs of a primary set of G shards into a replica set of H shards (created
    with FLAG_SHARD_REPLICA when H > 1).  A step drains every primary shard's ring on its device, routes the drain to the
    replicas' layout (Engine.records_route; skipped when the layouts are equal: shard i's log is then replica i's piece as it
    stands -- `routes` counts the route calls made), carries piece (i -> j) to replica j's device (`carry(tensor, engine)`;
    default `.to()` its device) and applies the pieces of destination j one after the other, folded or not.

    Per-row order holds under ANY order of the pieces: a key lives in exactly one source shard, so all records of a row are in
    one source's log, the route is stable, and pieces of different sources touch disjoint rows.

    `lost` is reported per source as LogShipper reports it; what a ring overwrote cannot be replayed.  `resync()` brings the
    replicas back from the primaries' tables through `resync_set` when the layouts are equal, and raises DintError when they
    are not (a resync pairs equal layouts; `reshard` moves tables between layouts)."""

    def __init__(self, primaries, replicas, cap: int = 1 << 20, chunk: int = 0, fold: bool = False, carry=None):
        import torch

        self.primaries, self.replicas = list(primaries), list(replicas)
        self.G, self.H = _layout(self.primaries), _layout(self.replicas)
        assert all(e.workload == self.primaries[0].workload for e in self.primaries + self.replicas)
        self.cap, self.chunk, self.fold = cap, chunk, fold
        self.carry = carry if carry is not None else (lambda t, e: t.to(e._torch_device()))
        self.bufs = [torch.empty(cap * LOG_REC.itemsize, dtype=torch.uint8, device=p._torch_device()) for p in self.primaries]
        self.outs = [torch.empty(cap * LOG_REC.itemsize, dtype=torch.uint8, device=p._torch_device()) for p in self.primaries] if self.G != self.H else []
        self.shipped = self.routes = self.resyncs = 0
        self.lost = [0] * self.G

    def step(self) -> dict:
        """one drain of every source and the replay of its pieces.  Returns {applied, commits / inserts / deletes (tatp) or acks
        (smallbank), folded / deferred (fold), lost: [per source], pieces: [(i, j, records)]}"""
        apply = apply_log_folded if self.fold else apply_log_device
        tot, pieces, lost = {}, [], []
        for i, p in enumerate(self.primaries):
            n, lo = p.log_drain_device(self.bufs[i], self.cap)
            lost.append(lo)
            self.lost[i] += lo
            self.shipped += n
            if n == 0:
                continue
            if self.G == self.H:
                parts = [(i, self.bufs[i][:n * LOG_REC.itemsize], n)]
            else:
                self.routes += 1
                parts = [(j, v, m) for j, (v, m) in enumerate(route_records(p, self.bufs[i], n, self.H, self.outs[i])) if m]
            for j, view, m in parts:
                r = self.replicas[j]
                st = apply(r, self.carry(view, r), m, self.chunk)
                pieces.append((i, j, m))
                for k, v in st.items():
                    tot[k] = tot.get(k, 0) + v
        tot.setdefault("applied", 0)
        tot["lost"], tot["pieces"] = lost, pieces
        return tot

    def resync(self, blocks=None) -> dict:
        """replicas := primaries, from the tables (see LogShipper.resync): every primary's drain cursor moves to its tail first."""
        if self.G != self.H:
            raise DintError(f"ShardSetShipper.resync: {self.G} primary shards, {self.H} replica shards: a resync pairs equal layouts; "
                            "recovery.reshard moves tables to another layout")
        for i, p in enumerate(self.primaries):
            while p.log_drain_device(self.bufs[i], self.cap)[0]:
                pass
        self.resyncs += 1
        return resync_set(self.primaries, self.replicas, blocks=blocks, cap=self.cap)
