// state_stats.h -- what a table's buckets and chains look like: one source for the kernels (k_stats.hip: dint_state_stats,
// include/dint_abi.h) and the host form over a state image (dint_state_stats_image_host, include/dint_driver.h), as
// state_image.h is for the image and state_rehash.h for the rehash.  Integer arithmetic only; nothing is written.
//
// One bucket is walked by state_image.h si_chain_walk, the one walk of the export, the check and the rehash: from the inline
// header's `head`, the inline entry an ordinary chain node wherever it sits and visited at most once, every other link checked
// by its owner (the pool's size / the bucket's run of the image's overflow section) before anything is read through it,
// KV_MAX_CHAIN entries at most.  A chain that cannot be walked contributes nothing but ST_BAD, and the caller refuses the
// whole report.
//
// A report is ST_WORDS 64-bit words, word for word the dint_table_stats of include/dint_abi.h:
//   buckets            local buckets
//   buckets_empty      ... without a valid slot
//   rows               valid slots reached by the walk
//   entries            entries linked into chains, the inline entry included when it is linked
//   overflow_entries   the pool entries among them
//   holes              4 * entries - rows
//   inline_first       buckets whose head == 1
//   inline_unlinked    buckets with a non-empty chain that does not contain the inline entry
//   hit_entries        over all valid slots: the 0-based position of the slot's entry in its chain + 1 (hit_entries / rows =
//                      the header sectors a lookup of a stored row walks, on average; shadowed rows count like any other)
//   shadowed_rows      valid slots whose key equals the key of an EARLIER valid slot of the bucket (chain order, entry after
//                      entry, slots 0..3).  Equal keys share a bucket: per table this is rows - distinct keys.  One lane's
//                      work is quadratic in the chain, so a bucket of more than ST_DUP_MAX_CHAIN entries is not compared:
//                      it adds 1 to buckets_unchecked and nothing here; all its other numbers are exact
//   longest_chain      entries of the longest chain;  longest_chain_bucket: the lowest GLOBAL bucket id that attains it
//                      (~0 for a table without rows: the answer never depends on scheduling);  most_rows: valid slots of the
//                      fullest bucket
//   chain_hist[17]     buckets by entries in the chain, 0..15, the last bin "16 or more"
//   rows_hist[33]      buckets by valid slots, 0..31, the last bin "32 or more"
//   locks_held         non-zero tatp lock bytes / smallbank {num_ex, num_sh} pairs with a non-zero word (state_image.h si_locks_held)
//   pool_cap, pool_top the table's control words (not part of an image: 0 there)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "state_image.h"

#define ST_DUP_MAX_CHAIN 64u  // entries of a bucket whose keys are still compared with each other
#define ST_CHAIN_BINS 17u
#define ST_ROWS_BINS 33u
#define ST_NO_BUCKET (~0ull)

enum : uint32_t {
  ST_BUCKETS = 0, ST_EMPTY, ST_ROWS, ST_ENTRIES, ST_OVERFLOW, ST_HOLES, ST_INLINE_FIRST, ST_INLINE_UNLINKED, ST_HIT, ST_SHADOWED,
  ST_UNCHECKED, ST_LONGEST, ST_LONGEST_BUCKET, ST_MOST_ROWS, ST_LOCKS, ST_POOL_CAP, ST_POOL_TOP,
  ST_CHAIN_HIST = 17,                          // .. 33
  ST_ROWS_HIST = ST_CHAIN_HIST + ST_CHAIN_BINS,  // 34 .. 66
  ST_BAD = ST_ROWS_HIST + ST_ROWS_BINS,          // 67: reserved[0] -- inside the implementation the buckets whose chain cannot be walked
  ST_WORDS = 80
};

// what one bucket adds
struct st_bucket {
  uint32_t rows, entries, overflow;
  uint32_t hit;        // <= 4 * KV_MAX_CHAIN * (KV_MAX_CHAIN + 1) / 2: 25 bits
  uint32_t shadowed, unchecked;
  uint32_t linked;     // the inline entry is part of the chain
  uint32_t first;      // ... and its head
  uint32_t ok;
};

SI_HD static inline uint32_t st_chain_bin(uint32_t entries) { return entries < ST_CHAIN_BINS - 1u ? entries : ST_CHAIN_BINS - 1u; }
SI_HD static inline uint32_t st_rows_bin(uint32_t rows) { return rows < ST_ROWS_BINS - 1u ? rows : ST_ROWS_BINS - 1u; }
SI_HD static inline bool st_slot_valid(uint32_t validw, uint32_t s) { return (validw >> (8 * s)) & 0xFFu; }
// is (chain, id) a better "longest chain" than (best, best_id)?  longer, or as long at a lower id
SI_HD static inline bool st_longer(uint64_t chain, uint64_t id, uint64_t best, uint64_t best_id) {
  return chain > best || (chain == best && id < best_id);
}

// A: si_chain_walk's accessor -- bool link_ok(link) for a link >= 2; void links(link, validw, next) for link 1 or an accepted
// link >= 2 -- with uint32_t head() and, for such a link, void keys(link, k[4]).
//
// the valid slots of the chain whose key an earlier valid slot holds.  Only called for a chain the walk below has found to
// end within ST_DUP_MAX_CHAIN entries; it re-walks instead of keeping the chain's keys (no array indexed at run time), and
// both loops are bounded whatever the links say by now.
template <class A>
SI_HD static inline uint32_t st_bucket_dups(const A &a, uint32_t head) {
  uint32_t dups = 0, li = head;
  for (uint32_t i = 0; i < ST_DUP_MAX_CHAIN && li != KV_NULL; i++) {
    if (li != KV_INLINE && !a.link_ok(li)) break;
    uint32_t vi, ni;
    a.links(li, vi, ni);
    if (vi) {
      uint64_t ki[4];
      a.keys(li, ki);
      uint32_t seen = 0;  // bit s: slot s repeats an earlier key
#pragma unroll
      for (uint32_t s = 1; s < 4; s++)
#pragma unroll
        for (uint32_t p = 0; p < s; p++)
          if (st_slot_valid(vi, s) && st_slot_valid(vi, p) && ki[s] == ki[p]) seen |= 1u << s;
      uint32_t lj = head;
      for (uint32_t j = 0; j < i && lj != KV_NULL; j++) {
        if (lj != KV_INLINE && !a.link_ok(lj)) break;
        uint32_t vj, nj;
        a.links(lj, vj, nj);
        if (vj) {
          uint64_t kj[4];
          a.keys(lj, kj);
#pragma unroll
          for (uint32_t s = 0; s < 4; s++)
#pragma unroll
            for (uint32_t p = 0; p < 4; p++)
              if (st_slot_valid(vi, s) && st_slot_valid(vj, p) && ki[s] == kj[p]) seen |= 1u << s;
        }
        lj = nj;
      }
      dups += (seen & 1u) + ((seen >> 1) & 1u) + ((seen >> 2) & 1u) + ((seen >> 3) & 1u);
    }
    li = ni;
  }
  return dups;
}

template <class A>
SI_HD static inline st_bucket st_bucket_walk(const A &a) {
  st_bucket r = {0, 0, 0, 0, 0, 0, 0, 0, 1};
  const uint32_t head = a.head();
  const bool ok = si_chain_walk(head, a, [&](uint32_t pos, uint32_t link, uint32_t validw) {
    if (link == KV_INLINE) r.linked = 1;
    else r.overflow++;
    const uint32_t c = si_valid_count(validw);
    r.rows += c;
    r.hit += c * (pos + 1u);
    r.entries++;
    return true;
  });
  if (!ok) return st_bucket{0, 0, 0, 0, 0, 0, 0, 0, 0};
  r.first = head == KV_INLINE;
  if (r.rows > 1) {  // (a key cannot repeat in a bucket of one row: no key vector is loaded there)
    if (r.entries > ST_DUP_MAX_CHAIN) r.unchecked = 1;
    else r.shadowed = st_bucket_dups(a, head);
  }
  return r;
}

// ---- a report as words ---------------------------------------------------------------------------------------------------
// the host form's accumulation (the kernel keeps the same sums in registers and LDS): w = ST_WORDS words, zero before the
// first bucket but for w[ST_LONGEST_BUCKET] = ST_NO_BUCKET
SI_HD static inline void st_report_init(uint64_t *w) {
  for (uint32_t k = 0; k < ST_WORDS; k++) w[k] = 0;
  w[ST_LONGEST_BUCKET] = ST_NO_BUCKET;
}
SI_HD static inline void st_report_add(uint64_t *w, const st_bucket &b, uint64_t global_id, uint32_t locks) {
  w[ST_BUCKETS]++;
  w[ST_LOCKS] += locks;
  if (!b.ok) {
    w[ST_BAD]++;
    return;
  }
  w[ST_EMPTY] += b.rows == 0;
  w[ST_ROWS] += b.rows;
  w[ST_ENTRIES] += b.entries;
  w[ST_OVERFLOW] += b.overflow;
  w[ST_INLINE_FIRST] += b.first;
  w[ST_INLINE_UNLINKED] += b.entries != 0 && !b.linked;
  w[ST_HIT] += b.hit;
  w[ST_SHADOWED] += b.shadowed;
  w[ST_UNCHECKED] += b.unchecked;
  if (b.entries && st_longer(b.entries, global_id, w[ST_LONGEST], w[ST_LONGEST_BUCKET])) {
    w[ST_LONGEST] = b.entries;
    w[ST_LONGEST_BUCKET] = global_id;
  }
  if (b.rows > w[ST_MOST_ROWS]) w[ST_MOST_ROWS] = b.rows;
  w[ST_CHAIN_HIST + st_chain_bin(b.entries)]++;
  w[ST_ROWS_HIST + st_rows_bin(b.rows)]++;
}
// what is derived once all buckets are in: the holes, and no bucket named for a table without rows.  Returns the buckets
// whose chain could not be walked (the report is refused when there is one) and clears that word.
SI_HD static inline uint64_t st_report_finish(uint64_t *w, uint64_t pool_cap) {
  const uint64_t bad = w[ST_BAD];
  w[ST_BAD] = 0;
  w[ST_HOLES] = 4 * w[ST_ENTRIES] - w[ST_ROWS];
  if (w[ST_ROWS] == 0) w[ST_LONGEST_BUCKET] = ST_NO_BUCKET;
  w[ST_POOL_CAP] = pool_cap;
  return bad;
}
