// state_verify.h -- is a table structurally sound?  An exact census of every chain, free list and pend list of one kv table
// and of its overflow pool, with the violations counted, and the one repair that needs no other information: putting leaked
// pool entries back on the free lists.  One source for the kernels (k_verify.hip: dint_state_verify, include/dint_abi.h) and
// the host form over caller-provided memory (dint_state_verify_view_host, include/dint_driver.h), as state_stats.h is for the
// table report.  Integer arithmetic only; the census writes nothing but its own owner words.  The engine is quiet meanwhile.
//
// OWNER WORDS.  Pool entry p of [0, pool_cap) has one uint32_t, zero at the start; non-zero = claimed.  A claim is
// compare-and-swap(owner[p], 0, code) -- the only atomic of the whole rule, on the entry's own word.  code = local bucket + 1
// for a chain (tables of SV_MAX_LOCAL or more local buckets are refused), SV_LIST_CODE + list for one of the SV_LISTS lists:
// the KV_NLISTS free lists first, then the two pend sets.
//
// CHAIN STAGE (complete before the list stage starts).  Each local bucket's chain is walked by state_image.h si_chain_walk
// under its bounds: KV_MAX_CHAIN entries, the inline entry at most once, a link >= 2 compared with pool_cap before anything is
// read through it.  Every overflow entry reached is claimed:
//   a new claim          linked++, and linked_beyond_top++ when p >= min(pool_top, pool_cap): each entry counts once there,
//                        for the walker that claimed it
//   another bucket's     cross_linked++; the walk goes on through the entry
//   this bucket's own    the chain has come back to an entry: it adds nothing a second time, and the walk's bound ends such
//                        a chain as a bad chain
// and for every entry reached, the inline one included, unless it is met again under the walker's own claim, the key vector is
// loaded when validw != 0 and per valid slot: rows++; misplaced_rows++ when the key is not home to this bucket (the accessor's
// home(): sr_local_bucket(fastmod(hash(key), hash_size), shard_index, shard_count)) -- counted by every walker, whoever holds
// the claim; odd_valid_bytes++ for a valid byte that is neither 0 nor 1 (dint_kv_core.h kv_valid takes it as valid, and so does
// this rule).  A chain that cannot be walked adds 1 to bad_chains; what it claimed and counted before stands.  A chain that
// ends without having met its inline entry, whose inline validw != 0: stray_valid_entries++, stray_rows += its valid slots.
//
// LIST STAGE.  Each list is followed from its head word {tag:32, link:32} through pool_next.  A link of 1 or beyond the pool:
// list_bad_links++, the walk ends, nothing is read through it.  Otherwise the entry is claimed; claimed already -- by a chain,
// another list or this list (a loop, two lists that merge, an entry freed but still linked) -- cross_linked++ and the walk ends:
// every step claims a fresh entry, so every walk is finite.  A new claim adds to free_entries or pending_entries, and to
// linked_beyond_top when p >= min(pool_top, pool_cap).  longest_list = the new claims of the longest walk.
//
// POOL STAGE.  Entry p < pool_cap: unclaimed below min(pool_top, pool_cap): unaccounted++ (handed out once, and now neither
// linked nor listed: leaked).  Not claimed by a chain and validw != 0: stray_valid_entries++, stray_rows += its valid slots (a
// flat scan such as the digest's counts them; no request finds them).  pool_top above pool_cap is reported raw and used clamped.
//
// Every number is exact and does not depend on scheduling while the structure is what the rule expects; with violations two
// things are not promised: how entries reachable from both a free and a pend list split between free_entries and
// pending_entries (their sum is), and, where lists merge or chains of several buckets share a loop, longest_list and the
// number of times the shared part adds to cross_linked.  Identities of every report: stray_rows >= stray_valid_entries, and,
// while cross_linked, bad_chains and list_bad_links are 0,
//   linked + free_entries + pending_entries - linked_beyond_top + unaccounted == min(pool_top, pool_cap).
//
// RECLAIM -- the one write; refused (not a byte written) while bad_chains, cross_linked, linked_beyond_top or list_bad_links
// is non-zero: the accounting cannot be trusted then.  U = the unaccounted entries ascending, n of them.  U[r] goes to free
// list r % KV_NLISTS: pool_next[U[r]] = U[r + KV_NLISTS] + 2 while r + KV_NLISTS < n, else the link half of the list's old
// head word; free_head[l] = {old tag + 1, U[l] + 2} for l < min(n, KV_NLISTS); the 8 bytes {validw, next} of every reclaimed
// header become zero and nothing else of an entry is touched.  The ranks come from a scan: no atomics.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "state_image.h"

#define SV_LISTS (3u * KV_NLISTS)       // free lists, pend set 0, pend set 1
#define SV_LIST_CODE 0xFFFFFF00u        // owner codes of the lists: SV_LIST_CODE + list
#define SV_MAX_LOCAL 0xFFFFFF00ull      // local buckets a table may have: a chain's code stays below the lists'
#define SV_CTL_TOP 0u                   // a table's control block: pool_top, ...
#define SV_CTL_HEADS 64u                // ... free_head[KV_NLISTS], pend_head[2][KV_NLISTS]: the SV_LISTS head words in list order
#define SV_CTL_BYTES (SV_CTL_HEADS + 8u * SV_LISTS)
static_assert(SV_LIST_CODE + SV_LISTS - 1u > SV_LIST_CODE && SV_MAX_LOCAL <= SV_LIST_CODE, "chain and list codes do not meet");

// a report: SV_WORDS 64-bit words, word for word the dint_table_verify of include/dint_abi.h
enum : uint32_t {
  SV_POOL_CAP = 0, SV_POOL_TOP, SV_ROWS, SV_LINKED, SV_FREE, SV_PENDING, SV_UNACCOUNTED, SV_LONGEST_LIST, SV_BAD_CHAINS, SV_CROSS,
  SV_BEYOND_TOP, SV_LIST_BAD_LINKS, SV_STRAY_ENTRIES, SV_STRAY_ROWS, SV_MISPLACED, SV_ODD_BYTES,
  SV_RECLAIMED,      // reserved[0]: with DINT_VERIFY_RECLAIM the entries put back on the free lists
  SV_STRAY_CLEARED,  // reserved[1]: ... and the valid slots their headers held
  SV_LEAKED_ROWS,    // inside the implementation: the valid slots of the unaccounted entries (0 in a finished report)
  SV_WORDS = 32
};
#define DINT_VERIFY_RECLAIM_BIT 1u  // = DINT_VERIFY_RECLAIM of include/dint_abi.h

SI_HD static inline bool sv_is_chain_code(uint32_t code) { return code != 0 && code < SV_LIST_CODE; }
SI_HD static inline uint32_t sv_chain_code(uint64_t bucket) { return (uint32_t)bucket + 1u; }
SI_HD static inline uint32_t sv_list_code(uint32_t list) { return SV_LIST_CODE + list; }
SI_HD static inline uint32_t sv_top(uint32_t pool_top, uint32_t pool_cap) { return pool_top < pool_cap ? pool_top : pool_cap; }
SI_HD static inline uint32_t sv_odd_bytes(uint32_t validw) {
  uint32_t n = 0;
  for (uint32_t s = 0; s < 4; s++) n += ((validw >> (8 * s)) & 0xFFu) > 1u;
  return n;
}

// ---- the chain stage: what one bucket adds --------------------------------------------------------------------------------------
struct sv_chain {
  uint32_t rows, linked, cross, beyond, bad, stray_entries, stray_rows, misplaced, odd;
};
// A: si_chain_walk's accessor over bucket b -- uint32_t head(); bool link_ok(link) for a link >= 2; void links(link, validw,
// next) and void keys(link, k[4]) for link 1 or an accepted link -- with
//   uint32_t inline_validw()       the inline entry's valid word
//   uint32_t claim(p, code)        compare-and-swap(owner[p], 0, code): what the word held before
//   uint64_t home(key)             the key's local bucket, or a value no local bucket has
// top = sv_top(pool_top, pool_cap)
template <class A>
SI_HD static inline sv_chain sv_chain_stage(const A &a, uint64_t b, uint32_t top) {
  sv_chain r = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const uint32_t code = sv_chain_code(b);
  bool inl = false;
  const bool ok = si_chain_walk(a.head(), a, [&](uint32_t, uint32_t link, uint32_t validw) {
    if (link == KV_INLINE) {
      inl = true;
    } else {
      const uint32_t p = link - 2u, was = a.claim(p, code);
      if (was == 0) {
        r.linked++;
        r.beyond += p >= top;
      } else if (was == code) {
        return true;  // met again: counted already
      } else {
        r.cross++;
      }
    }
    if (validw) {
      uint64_t k[4];
      a.keys(link, k);
#pragma unroll
      for (uint32_t s = 0; s < 4; s++)
        if ((validw >> (8 * s)) & 0xFFu) {
          r.rows++;
          r.misplaced += a.home(k[s]) != b;
        }
      r.odd += sv_odd_bytes(validw);
    }
    return true;
  });
  if (!ok) {
    r.bad = 1;
  } else if (!inl) {
    const uint32_t v = a.inline_validw();
    if (v) {
      r.stray_entries = 1;
      r.stray_rows = si_valid_count(v);
    }
  }
  return r;
}

// ---- the list stage: what one list adds -----------------------------------------------------------------------------------------
struct sv_list {
  uint32_t claimed, cross, beyond, bad_links;
};
// L: uint32_t pool_next(p) for p < pool_cap; uint32_t claim(p, code).  head_link = the link half of the list's head word
template <class L>
SI_HD static inline sv_list sv_list_stage(const L &l, uint32_t list, uint32_t head_link, uint32_t pool_cap, uint32_t top) {
  sv_list r = {0, 0, 0, 0};
  const uint32_t code = sv_list_code(list);
  uint32_t link = head_link;
  while (link != KV_NULL) {
    if (link - 2u >= pool_cap) {  // (link 1 wraps around to the largest number)
      r.bad_links = 1;
      break;
    }
    const uint32_t p = link - 2u;
    if (l.claim(p, code) != 0) {
      r.cross = 1;
      break;
    }
    r.claimed++;  // (a fresh entry every step: at most pool_cap steps)
    r.beyond += p >= top;
    link = l.pool_next(p);
  }
  return r;
}
SI_HD static inline bool sv_list_is_free(uint32_t list) { return list < KV_NLISTS; }

// ---- the pool stage: what one pool entry adds -------------------------------------------------------------------------------------
struct sv_pool {
  uint32_t unaccounted, stray_entries, stray_rows, leaked_rows;
};
SI_HD static inline sv_pool sv_pool_entry(uint32_t p, uint32_t owner, uint32_t validw, uint32_t top) {
  sv_pool r = {0, 0, 0, 0};
  r.unaccounted = owner == 0 && p < top;
  if (!sv_is_chain_code(owner) && validw) {
    r.stray_entries = 1;
    r.stray_rows = si_valid_count(validw);
    if (r.unaccounted) r.leaked_rows = r.stray_rows;
  }
  return r;
}

// ---- a report as words ------------------------------------------------------------------------------------------------------------
SI_HD static inline void sv_report_add_chain(uint64_t *w, const sv_chain &c) {
  w[SV_ROWS] += c.rows; w[SV_LINKED] += c.linked; w[SV_CROSS] += c.cross; w[SV_BEYOND_TOP] += c.beyond; w[SV_BAD_CHAINS] += c.bad;
  w[SV_STRAY_ENTRIES] += c.stray_entries; w[SV_STRAY_ROWS] += c.stray_rows; w[SV_MISPLACED] += c.misplaced; w[SV_ODD_BYTES] += c.odd;
}
SI_HD static inline void sv_report_add_list(uint64_t *w, uint32_t list, const sv_list &l) {
  w[sv_list_is_free(list) ? SV_FREE : SV_PENDING] += l.claimed;
  w[SV_CROSS] += l.cross; w[SV_BEYOND_TOP] += l.beyond; w[SV_LIST_BAD_LINKS] += l.bad_links;
  if (l.claimed > w[SV_LONGEST_LIST]) w[SV_LONGEST_LIST] = l.claimed;
}
SI_HD static inline void sv_report_add_pool(uint64_t *w, const sv_pool &p) {
  w[SV_UNACCOUNTED] += p.unaccounted; w[SV_STRAY_ENTRIES] += p.stray_entries; w[SV_STRAY_ROWS] += p.stray_rows;
  w[SV_LEAKED_ROWS] += p.leaked_rows;
}
// may the unaccounted entries of this census go back to the free lists?
SI_HD static inline bool sv_reclaim_ok(const uint64_t *w) {
  return (w[SV_BAD_CHAINS] | w[SV_CROSS] | w[SV_BEYOND_TOP] | w[SV_LIST_BAD_LINKS]) == 0;
}
// what the caller sees of the words once everything is in; reclaimed: the unaccounted entries went back to the free lists
SI_HD static inline void sv_report_finish(uint64_t *w, bool reclaimed) {
  w[SV_RECLAIMED] = reclaimed ? w[SV_UNACCOUNTED] : 0;
  w[SV_STRAY_CLEARED] = reclaimed ? w[SV_LEAKED_ROWS] : 0;
  w[SV_LEAKED_ROWS] = 0;
}

// ---- reclaim ----------------------------------------------------------------------------------------------------------------------
// pool_next of U[r]: ahead = U[r + KV_NLISTS] (only read while r + KV_NLISTS < n), old_head = the old head word of list r % KV_NLISTS
SI_HD static inline uint32_t sv_reclaim_next(uint64_t r, uint64_t n, uint32_t ahead, uint64_t old_head) {
  return r + KV_NLISTS < n ? ahead + 2u : (uint32_t)old_head;
}
// the new head word of a list that takes `first` = U[l]
SI_HD static inline uint64_t sv_reclaim_head(uint64_t old_head, uint32_t first) { return ((old_head >> 32) + 1ull) << 32 | (uint64_t)(first + 2u); }
