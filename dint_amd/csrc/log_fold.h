// log_fold.h -- a chunk of a drained log folded to its net effect per row, one source for the host form (dint_log_fold_host,
// include/dint_driver.h) and the fold kernels (k_fold.hip), as log_replay.h is for the replay and state_compact.h for the
// compaction.  Integer arithmetic only, so host and device choose the same bytes.
//
// The serial replay (k_replay.hip) turns every record into a backup operation and lets the hot path resolve thousands of writes
// to one row in request order; all that survives is the row's last value and a version that follows from a count.  The fold
// computes that directly and hands it to the state repair (k_state.hip k_state_repair), which writes "this row, this value, this
// version / this row gone" with one lane per bucket.  The target: afterwards every table holds the multiset of rows (key, version,
// value) that dint_log_apply_device leaves on the same replica, the same records and the same chunk.
//
// Per chunk of records r[0 .. m) in log order, the replica's tables taken as they are when the chunk starts:
//   row     (table, key); bucket = fasthash64(key) % hash_size[table].  Rows are grouped through log_replay.h lr_row, so keys
//           stay below 2^60 as they do there.
//   occ     the valid slots of the bucket's chain -- inline entry and overflow entries -- that hold the key;
//   v0      the version of the visible one, the first in chain order.
//   A bucket is DEFERRED if any row of it that the chunk touches has occ >= 2, and so is every record of the bucket, whatever its
//   key: with a duplicate in the chain, which row a later COMMIT_BCK hits depends on where an INSERT_BCK lands, and that on the
//   holes other keys of the bucket leave.  Only the serial order gets that right, so those records go through the serial replay in
//   log order.  A record that names a table the workload has not is deferred too: the serial replay answers it as it always did.
//   A bucket that is not deferred cannot become duplicated during the chunk: the replay calls a record INSERT_BCK only after a
//   delete or after a probe that found nothing.
//
//   A folded row has records 1 .. k in log order; d = the index of the last one with is_del set (0: none), c = k - d.
//   tatp       c == 0: the row is gone -- a delete if occ == 1, nothing if occ == 0.
//              c > 0:  {val = the last record's, ver}; ver = v0 + c when d == 0 and occ == 1 (c commits on the row as it was),
//                      else c - 1 (re-inserted at version 0 after the delete, or inserted because it was absent, then c - 1
//                      commits).  u32 arithmetic, wrapping as the version word does.
//   smallbank  every record is a COMMIT_BCK: k_replay.hip does not look at is_del for smallbank, and neither does the fold
//              (d = 0).  occ == 0: nothing (kvs_set on a missing key leaves the table alone); else {val = the last record's
//              first 8 bytes, ver = v0 + k}.
//   What the records would have been as backup operations (the stats): record j of a row is a delete if is_del is set (tatp),
//   else a commit if the row exists before it -- j == 1: occ >= 1; else log_replay.h lr_exists_after of record j - 1 -- else an
//   insert.
//
// The last delete of a row comes from an inclusive max-scan over the sorted positions of "p + 1 if the record at p is a delete,
// else 0".  Positions only grow, so the scan needs no segment flags: a maximum carried in from an earlier row is a position below
// the row's first and is read as "none" (lf_last_delete) -- the segmented scan's answer with a plain operator.
#pragma once
#include <stdint.h>

#include "log_replay.h"

#define LF_HD LR_HD

enum : uint32_t { LF_NONE = 0, LF_DELETE = 1, LF_PUT = 2 };       // what a folded row hands to the repair
enum : uint32_t { LF_COMMIT = 0, LF_INSERT = 1, LF_DEL = 2 };    // a record as a backup operation (the stats)
#define LF_BAD_TABLE 7u   // the table code, in a place word, of a record whose table the workload has not (tables are < 5)
#define LF_PLACE_BITS 35u // bits of a place word: 32 of the bucket, 3 of the table

// where a record's bucket sorts: ascending (table, bucket), the order k_state_repair_check demands
LF_HD static inline uint64_t lf_place(uint32_t table, uint64_t bucket) { return ((uint64_t)table << 32) | (bucket & 0xFFFFFFFFull); }
LF_HD static inline uint32_t lf_place_table(uint64_t place) { return (uint32_t)(place >> 32); }
LF_HD static inline uint32_t lf_place_bucket(uint64_t place) { return (uint32_t)place; }

// d of a row whose records sit at sorted positions [s, ..]: scan = the max-scan's value at the row's last position
LF_HD static inline uint32_t lf_last_delete(uint32_t scan, uint32_t s) { return scan > s ? scan - s : 0u; }

// does the bucket of a row with this occ go the serial way?
LF_HD static inline bool lf_defers(uint32_t occ) { return occ >= 2u; }

struct lf_net {
  uint32_t kind;  // LF_NONE / LF_DELETE / LF_PUT
  uint32_t ver;   // of an LF_PUT
};
// the net effect of a folded row: k records, the last delete at index d (1-based, 0 = none; smallbank: pass 0)
LF_HD static inline lf_net lf_fold(bool smallbank, uint32_t occ, uint32_t v0, uint32_t k, uint32_t d) {
  if (smallbank) return occ == 0 ? lf_net{LF_NONE, 0u} : lf_net{LF_PUT, v0 + k};
  const uint32_t c = k - d;
  if (c == 0) return occ == 1 ? lf_net{LF_DELETE, 0u} : lf_net{LF_NONE, 0u};
  return lf_net{LF_PUT, (d == 0 && occ == 1) ? v0 + c : c - 1u};
}

// record j of a row as a backup operation: first = j == 1, prev_is_del = is_del of record j - 1 (not read when first)
LF_HD static inline uint32_t lf_kind(bool smallbank, uint8_t is_del, bool first, uint32_t occ, uint8_t prev_is_del) {
  if (smallbank) return LF_COMMIT;
  if (is_del) return LF_DEL;
  return (first ? occ >= 1u : lr_exists_after(prev_is_del)) ? LF_COMMIT : LF_INSERT;
}

// the 64-byte repair record as sixteen words; last = the sixteen words of the row's last record (read for an LF_PUT only).
// Bytes the rule does not name are zero.
LF_HD static inline void lf_record(uint32_t w[16], bool smallbank, lf_net net, uint64_t key, uint32_t table, const uint32_t last[16]) {
  for (int i = 0; i < 16; i++) w[i] = 0;
  w[0] = (uint32_t)key;
  w[1] = (uint32_t)(key >> 32);
  if (net.kind == LF_PUT) {
    const int words = smallbank ? 2 : 10;  // val = bytes 8 .. 48 of a record
    for (int i = 0; i < words; i++) w[2 + i] = last[2 + i];
    w[12] = net.ver;
    w[13] = table << 8;
  } else {
    w[13] = 1u | (table << 8);
  }
}
