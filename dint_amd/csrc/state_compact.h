// state_compact.h -- a table compacted IN PLACE: state_rehash.h's layout rule applied to one engine onto itself, at the same
// bucket count and shard, so no row changes its bucket and the lock words in the inline entries can stay where they are.  One
// source for the kernels (k_compact.hip: dint_state_compact, include/dint_abi.h) and the host form over caller-provided memory
// (dint_state_compact_view_host, include/dint_driver.h), as state_verify.h is for the census.  Integer arithmetic only.
//
// THE GATE.  state_verify.h's census runs first.  Nothing is written while bad_chains, cross_linked, linked_beyond_top,
// list_bad_links, stray_valid_entries, misplaced_rows or odd_valid_bytes is non-zero in ANY table (cp_gate_ok): the chains
// cannot be trusted then.  Leaked (unaccounted) entries are no violation: compaction drops them.
//
// PLACEMENT.  For every local bucket the k valid rows in chain order (head first, slots 0 .. 3 inside an entry) are rows
// r = 0 .. k - 1.  Row r goes to chain position sr_chain_pos(r), slot sr_slot(r).  Chain position 0 is the inline entry (head =
// KV_INLINE), chain position x >= 1 pool entry base[b] + x - 1, base = the exclusive scan of sr_overflow(k) over the local
// buckets ascending, starting at 0.  Key, version and value are copied verbatim; a valid byte is 1; unused slots of a used entry
// (key, version, value, valid byte) are zero.  An empty bucket has head = 0 and its inline validw and next zero, and its four
// slots are unused slots like any other: zero, whatever deleted rows left there (so an engine without lock words exports the same
// image as a blank twin it was rehashed into).  In an INLINE entry lockw, smallbank's counter pairs (KV_SB_LOCK_OFF) and tatp's
// owner keys (KV_OWNER_OFF) keep their bytes; in an overflow entry the same bytes, and `head`, are zero.
//
// THE POOL AFTERWARDS.  pool_top = the sum of the overflow counts.  Every one of the SV_LISTS head words becomes {tag + 1, 0}.
// Pool entries [new top, min(old top, pool_cap)) get their 8 bytes {validw, next} zeroed; pool_next[] is not touched (no list
// is left to read it).  Dropped with the holes: entries without a valid slot, leaked entries, everything on the lists.
//
// ORDER.  Two rows of one key share their bucket and keep their order, so every key's visible row stays its visible row.
//
// A bucket cannot rewrite itself in place: its new pool entries are other buckets' old ones.  So overflow entries go to a
// STAGING buffer (zero at the start) at their final index first, the inline entry is written once the bucket's first four rows
// have been read -- only the bucket itself reads its own inline entry in a table that passed the gate -- and the staging buffer
// is copied over pool entries [0, new top) when every bucket has been read.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "state_image.h"
#include "state_rehash.h"
#include "state_verify.h"

// a report: the census's SV_WORDS words, then these; word for word the dint_table_compact of include/dint_abi.h
enum : uint32_t {
  CP_ROWS = SV_WORDS, CP_ENTRIES_BEFORE, CP_ENTRIES_AFTER, CP_OVERFLOW_BEFORE, CP_OVERFLOW_AFTER, CP_TOP_BEFORE, CP_TOP_AFTER,
  CP_HOLES_BEFORE, CP_HOLES_AFTER, CP_REWRITTEN, CP_DROPPED, CP_STAGING_BYTES,
  CP_STAGE_NS,  // reserved[0 .. 3] of table 0, with timing on: census, count and scans, move, commit
  CP_WORDS = 64
};
#define DINT_COMPACT_DRY_RUN_BIT 1u  // = DINT_COMPACT_DRY_RUN of include/dint_abi.h
// what the count stage sums per table (the device keeps them as four words)
enum : uint32_t { CP_SUM_OVERFLOW = 0, CP_SUM_REWRITTEN, CP_SUM_INLINE_LINKED, CP_SUM_NONEMPTY, CP_SUMS };

// may a table with this census be compacted?
SI_HD static inline bool cp_gate_ok(const uint64_t *w) {
  return (w[SV_BAD_CHAINS] | w[SV_CROSS] | w[SV_BEYOND_TOP] | w[SV_LIST_BAD_LINKS] | w[SV_STRAY_ENTRIES] | w[SV_MISPLACED] | w[SV_ODD_BYTES]) == 0;
}

// ---- the count stage: what one bucket is now ------------------------------------------------------------------------------------
struct cp_count {
  uint32_t k;              // valid rows of the chain
  uint32_t inline_linked;  // the inline entry is part of the chain
  uint32_t rewritten;      // the chain is not yet what the rule makes of it: inline entry first, every entry full but the last,
                           // the last one's rows in its first slots; an empty bucket: head != KV_NULL
  uint32_t ok;             // the walk reached the end of the chain
};
// A: si_chain_walk's accessor -- uint32_t head(); bool link_ok(link); void links(link, validw, next)
template <class A>
SI_HD static inline cp_count cp_count_bucket(const A &a) {
  cp_count c = {0, 0, 0, 1};
  const uint32_t head = a.head();
  uint32_t last = 0x01010101u, entries = 0;
  bool dense = true;
  c.ok = si_chain_walk(head, a, [&](uint32_t, uint32_t link, uint32_t validw) {
    if (link == KV_INLINE) c.inline_linked = 1;
    dense = dense && last == 0x01010101u;  // (every entry ahead of this one is full)
    last = validw;
    entries++;
    c.k += si_valid_count(validw);
    return true;
  });
  if (c.k == 0) c.rewritten = head != KV_NULL;
  else c.rewritten = !(head == KV_INLINE && dense && entries == sr_entries(c.k) && last == sr_validw(c.k - 4u * (entries - 1u)));
  return c;
}

// ---- the move stage: one bucket rewritten ---------------------------------------------------------------------------------------
struct cp_loc {
  uint32_t link, slot;
};
// the link words of the entry at chain position x of a bucket of k rows whose overflow entries start at pool entry `base`
SI_HD static inline uint32_t cp_validw(uint32_t k, uint32_t x) { return sr_validw(k - 4u * x < 4u ? k - 4u * x : 4u); }
SI_HD static inline uint32_t cp_next(uint32_t k, uint32_t x, uint32_t base) { return x + 1u < sr_entries(k) ? sr_link(x + 1u, base + x) : KV_NULL; }
// A: the accessor above, with
//   void stage_row(src_link, src_slot, pool, slot)   key, version and value of a row into staging entry `pool`, slot `slot`
//   void stage_links(pool, validw, next)             the link words of staging entry `pool`
//   void inline_write(loc[4], m, validw, next, head) the bucket's inline entry := rows loc[0 .. m) in slots 0 .. m - 1, the other
//                                                    slots zero, {validw, next, head}; every load before the first store
// k = cp_count_bucket's, base = the bucket's first overflow entry.  Never more than k rows are placed, whatever the chain holds
// now: a staging entry outside [base, base + sr_overflow(k)) is never written.
template <class A>
SI_HD static inline void cp_move_bucket(const A &a, uint32_t k, uint32_t base) {
  cp_loc loc[4] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
  if (k == 0) {
    a.inline_write(loc, 0u, 0u, KV_NULL, KV_NULL);
    return;
  }
  uint32_t r = 0;
  (void)si_chain_walk(a.head(), a, [&](uint32_t, uint32_t link, uint32_t validw) {
#pragma unroll
    for (uint32_t s = 0; s < 4; s++) {
      if (!((validw >> (8 * s)) & 0xFFu) || r >= k) continue;
      if (r < 4u) {
#pragma unroll
        for (uint32_t i = 0; i < 4; i++)
          if (i == r) loc[i] = cp_loc{link, s};
      } else {
        const uint32_t x = sr_chain_pos(r), pool = base + x - 1u;
        if (sr_opens_entry(r)) a.stage_links(pool, cp_validw(k, x), cp_next(k, x, base));
        a.stage_row(link, s, pool, sr_slot(r));
      }
      r++;
    }
    return r < k;
  });
  a.inline_write(loc, r < 4u ? r : 4u, cp_validw(k, 0), cp_next(k, 0, base), KV_INLINE);
}

// ---- a report as words ------------------------------------------------------------------------------------------------------------
// w = a table's finished census (SV_WORDS words) with room for CP_WORDS; sums = the count stage's CP_SUMS totals; moved = the gate
// let the compaction through (or would have: a dry run).  A refused table reports its census and zeros.
SI_HD static inline void cp_report_finish(uint64_t *w, const uint64_t *sums, uint32_t stride, bool moved) {
  for (uint32_t i = SV_WORDS; i < CP_WORDS; i++) w[i] = 0;
  if (!moved) return;
  w[CP_ROWS] = w[SV_ROWS];
  w[CP_OVERFLOW_BEFORE] = w[SV_LINKED];
  w[CP_ENTRIES_BEFORE] = w[SV_LINKED] + sums[CP_SUM_INLINE_LINKED];
  w[CP_OVERFLOW_AFTER] = sums[CP_SUM_OVERFLOW];
  w[CP_ENTRIES_AFTER] = sums[CP_SUM_OVERFLOW] + sums[CP_SUM_NONEMPTY];
  w[CP_TOP_BEFORE] = w[SV_POOL_TOP];
  w[CP_TOP_AFTER] = sums[CP_SUM_OVERFLOW];
  w[CP_HOLES_BEFORE] = 4u * w[CP_ENTRIES_BEFORE] - w[CP_ROWS];
  w[CP_HOLES_AFTER] = 4u * w[CP_ENTRIES_AFTER] - w[CP_ROWS];
  w[CP_REWRITTEN] = sums[CP_SUM_REWRITTEN];
  w[CP_DROPPED] = w[SV_UNACCOUNTED];
  w[CP_STAGING_BYTES] = sums[CP_SUM_OVERFLOW] * (uint64_t)stride;
}
