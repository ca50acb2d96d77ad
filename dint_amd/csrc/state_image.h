// state_image.h -- the position-independent image of an engine's tables: one source for the kernels (k_image.hip:
// dint_state_export / dint_state_import, include/dint_abi.h) and the host form (dint_state_image_check_host,
// include/dint_driver.h), as state_sync.h is for the state sync.
//
// An image holds everything of ONE source engine (src_index, src_count) that belongs to ONE destination shard
// (dst_index, dst_count): the global buckets / slots g the source owns with g % dst_count == dst_index, entry for entry.
// All integers little-endian; every section starts on a 16-byte boundary.
//
//   header   SI_HEADER_BYTES (320): si_header -- magic "DINTIMG1", version, workload, the layout-relevant flags
//            (DINT_FLAG_LOCK_SAME_KEY), tables, stride, value size, source and destination (index, count), the image's
//            size, and per table {global hash size or n_slots, buckets, overflow entries, valid slots, offset}
//   per kv table, at its offset:
//     dir      buckets x 16 bytes  {u64 global bucket, u32 first, u32 count}: ascending global buckets; [first, first +
//              count) is the bucket's run of overflow entries below, the runs laid end to end in bucket order
//     inline   buckets x stride    the inline entries, verbatim (keys, versions, valid bytes, values, tatp lock bytes,
//              smallbank counters, owner keys), but for the two link words
//     overflow entries x stride    every bucket's overflow entries in CHAIN order, verbatim but for `next`
//   links (`head` of an inline entry, `next` of every entry) are image-relative: 0 = end, 1 = the bucket's inline entry,
//   k >= 2 = overflow entry k - 2 of this table's section.  The chain of a bucket visits its run exactly once and in order,
//   so an overflow entry's successor, when it is an overflow entry, is simply the next one; the inline entry stays wherever
//   it was in the chain (or outside it: then it holds no valid slot, and its `next` is written as 0).  Invalid slots and
//   shadowed duplicates are where they were.
//   lock tables (lock_fasst / lock_2pl): one table of slots x 16 bytes {u64 global slot, u32 a, u32 b}, ascending.
// Not in an image: the log ring, the pool's free and pend lists, pass scratch.
//
// Import adds one number to every link >= 2: the image's overflow entries become ONE contiguous range of the pool.
// Nothing of an image is trusted (it may come from a file): si_header_check and si_check_bucket / si_check_slot say whether
// it can be imported without reading or writing outside the image and the tables.  Integer arithmetic only.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/dint_abi.h"
#include "dint_kv_core.h"

#if defined(__HIPCC__)
#define SI_HD __host__ __device__
#else
#define SI_HD
#endif

#define SI_MAGIC 0x31474D49544E4944ULL  // "DINTIMG1"
#define SI_VERSION 1u
#define SI_HEADER_BYTES 320u
#define SI_MAX_TABLES 5u
#define SI_LOCK_STRIDE 8u                 // header.stride of a lock table's image (a uint2 slot)
#define SI_MAX_RUN (KV_MAX_CHAIN - 1u)    // overflow entries of one bucket: the whole chain stays within every walk's bound
#define SI_LINK_VEC 3u                    // the 16-byte vector of an entry that holds {validw, next, head, lockw}

struct si_table {
  uint64_t global_size;  // kv: the table's global bucket count; lock tables: n_slots
  uint64_t n_buckets;    // buckets / slots in the image
  uint64_t n_overflow;   // overflow entries in the image
  uint64_t rows;         // valid slots (lock tables: slots with a non-zero word)
  uint64_t offset;       // of the table's section in the image
};
struct si_header {
  uint64_t magic;
  uint32_t version, workload, flags, n_tables, stride, val_size;
  uint32_t src_index, src_count, dst_index, dst_count;
  uint64_t bytes;
  uint64_t reserved;
  si_table table[SI_MAX_TABLES];
  uint8_t pad[56];
};
static_assert(sizeof(si_header) == SI_HEADER_BYTES && offsetof(si_header, table) == 64, "image header layout");
struct si_dir {
  uint64_t id;
  uint32_t first, count;  // (lock tables: the slot's two words)
};
static_assert(sizeof(si_dir) == 16, "one 16-byte vector per bucket");
static_assert(offsetof(kv_hdr, validw) == 16 * SI_LINK_VEC && offsetof(kv_hdr, next) == 16 * SI_LINK_VEC + 4 &&
              offsetof(kv_hdr, head) == 16 * SI_LINK_VEC + 8, "the link words share one vector");

// what a check found (a bit each; the lowest bit set is the first violation in the order the rule is applied)
enum : uint32_t {
  SI_BAD_SIZE = 1u,       // the sizes in the header do not add up to `bytes`
  SI_BAD_ORDER = 2u,      // ids not strictly ascending
  SI_BAD_RANGE = 4u,      // an id beyond the table
  SI_BAD_HOME = 8u,       // an id that is not the source's or not the destination's
  SI_BAD_RUN = 16u,       // the runs of overflow entries are not laid end to end, or one is longer than a chain may be
  SI_BAD_LINK = 32u,      // a link that is not 0, 1 or inside its own bucket's run
  SI_BAD_CHAIN = 64u,     // the chain does not visit the bucket's run exactly once and in order
  SI_BAD_UNLINKED = 128u  // an inline entry outside its chain that holds valid slots
};
SI_HD static inline const char *si_bad_name(uint32_t bad) {
  if (bad & SI_BAD_SIZE) return "the sizes in the header are not consistent with the image's bytes";
  if (bad & SI_BAD_ORDER) return "ids not strictly ascending";
  if (bad & SI_BAD_RANGE) return "an id out of range";
  if (bad & SI_BAD_HOME) return "an id that is not home to the image's source and destination";
  if (bad & SI_BAD_RUN) return "the buckets' runs of overflow entries are not laid end to end";
  if (bad & SI_BAD_LINK) return "a link beyond its bucket's run of overflow entries";
  if (bad & SI_BAD_CHAIN) return "a chain that skips or revisits an entry of its bucket's run";
  if (bad & SI_BAD_UNLINKED) return "an inline entry outside its chain holds valid slots";
  return "nothing";
}

SI_HD static inline uint32_t si_valid_count(uint32_t validw) {
  return ((validw & 0xFFu) != 0) + ((validw & 0xFF00u) != 0) + ((validw & 0xFF0000u) != 0) + ((validw & 0xFF000000u) != 0);
}
// lock words live in the inline header of a bucket, and where depends on the workload
enum : uint32_t {
  SI_LOCKS_NONE = 0,      // store
  SI_LOCKS_TATP = 1,      // the four lock bytes of the header's word at KV_LOCKB_OFF
  SI_LOCKS_SMALLBANK = 2  // four {num_ex, num_sh} pairs at KV_SB_LOCK_OFF
};
SI_HD static inline uint32_t si_lock_mode(uint32_t workload) {
  return workload == DINT_WL_TATP ? SI_LOCKS_TATP : workload == DINT_WL_SMALLBANK ? SI_LOCKS_SMALLBANK : SI_LOCKS_NONE;
}
// lock words held by one inline header: non-zero tatp lock bytes of `lockw` / smallbank pairs with a non-zero word
// (counters(c) fills c[8] with the header's eight counter words; only called for smallbank)
template <class C>
SI_HD static inline uint32_t si_locks_held(uint32_t lock_mode, uint32_t lockw, C &&counters) {
  if (lock_mode == SI_LOCKS_TATP) return si_valid_count(lockw);  // (non-zero bytes of the word)
  if (lock_mode != SI_LOCKS_SMALLBANK) return 0;
  uint32_t c[8];
  counters(c);
  return ((c[0] | c[1]) != 0) + ((c[2] | c[3]) != 0) + ((c[4] | c[5]) != 0) + ((c[6] | c[7]) != 0);
}
SI_HD static inline uint64_t si_gcd(uint64_t a, uint64_t b) {
  while (b) { const uint64_t r = a % b; a = b; b = r; }
  return a;
}

// ---- which local buckets of a source (i, G) belong to destination (j, H) ---------------------------------------------
// local bucket l of the source is global bucket l * G + i; the selected ones are l0, l0 + step, ... (n of them)
struct si_sel {
  uint64_t l0, step, n;
  uint32_t G, i;
};
SI_HD static inline si_sel si_select(uint64_t global_size, uint32_t i, uint32_t G, uint32_t j, uint32_t H) {
  si_sel s = {0, 1, 0, G, i};
  const uint64_t g = si_gcd(G, H);
  s.step = H / g;
  if (i % g != j % g || global_size <= i) return s;  // (an empty piece)
  const uint64_t n_local = (global_size - i + G - 1) / G;  // the source's local buckets that exist globally
  for (s.l0 = 0; s.l0 < s.step; s.l0++)
    if ((s.l0 * G + i) % H == j) break;
  if (s.l0 < n_local) s.n = (n_local - s.l0 + s.step - 1) / s.step;
  return s;
}

// ---- the header ----------------------------------------------------------------------------------------------------
// bytes of a table's section / the offsets of its three parts
SI_HD static inline uint64_t si_table_bytes(uint64_t n_buckets, uint64_t n_overflow, uint32_t stride, bool lock) {
  return lock ? 16 * n_buckets : 16 * n_buckets + (n_buckets + n_overflow) * (uint64_t)stride;
}
// the header's own consistency (not its match with an engine): SI_BAD_SIZE or 0.  After this every section lies inside
// [0, bytes) and no product below overflows.
SI_HD static inline uint32_t si_header_check(const si_header &h, uint64_t bytes, bool lock) {
  if (bytes < SI_HEADER_BYTES || h.magic != SI_MAGIC || h.version != SI_VERSION || h.bytes != bytes) return SI_BAD_SIZE;
  if (h.n_tables == 0 || h.n_tables > SI_MAX_TABLES || h.src_count == 0 || h.dst_count == 0 || h.src_count > 255 || h.dst_count > 255 ||
      h.src_index >= h.src_count || h.dst_index >= h.dst_count)
    return SI_BAD_SIZE;
  if (lock ? h.stride != SI_LOCK_STRIDE : (h.stride != 256 && h.stride != 128)) return SI_BAD_SIZE;
  uint64_t at = SI_HEADER_BYTES;
  for (uint32_t t = 0; t < h.n_tables; t++) {
    const si_table &tb = h.table[t];
    if (tb.offset != at || tb.n_buckets > bytes / 16 || tb.n_overflow > bytes / h.stride || (lock && tb.n_overflow) ||
        tb.n_overflow > 0xFFFFFFF0ull || tb.global_size == 0 || (tb.n_buckets == 0 && tb.n_overflow))  // (overflow entries belong to a bucket's run)
      return SI_BAD_SIZE;
    const uint64_t sz = si_table_bytes(tb.n_buckets, tb.n_overflow, h.stride, lock);
    if (sz > bytes - at) return SI_BAD_SIZE;
    at += sz;
  }
  return at == bytes ? 0 : SI_BAD_SIZE;
}

// ---- the link rules ------------------------------------------------------------------------------------------------
// out (export).  The overflow entry that becomes image entry x: chain order is image order, so a successor in the pool
// is entry x + 1.
SI_HD static inline uint32_t si_next_out(uint32_t src_next, uint64_t x) { return src_next >= 2u ? (uint32_t)(x + 1) + 2u : src_next; }
// ... the inline entry of a bucket whose run starts at `first`, with `before` overflow entries ahead of it in the chain
SI_HD static inline uint32_t si_head_out(uint32_t src_head, uint64_t first) { return src_head >= 2u ? (uint32_t)first + 2u : src_head; }
SI_HD static inline uint32_t si_inline_next_out(uint32_t src_next, bool linked, uint64_t first, uint32_t before) {
  if (!linked) return 0;  // (a stale link of an entry outside its chain: never read, not carried)
  return src_next >= 2u ? (uint32_t)(first + before) + 2u : src_next;
}
// in (import): the image's overflow entries are pool entries [base, base + n_overflow)
SI_HD static inline uint32_t si_link_in(uint32_t link, uint32_t base) { return link >= 2u ? link + base : link; }

// ---- one chain, wherever it lies --------------------------------------------------------------------------------------
// THE walk of a bucket's chain, for tables in HBM and images alike: from `head` to KV_NULL, KV_MAX_CHAIN entries at most, the
// inline entry (link KV_INLINE) an ordinary chain node wherever it sits and visited at most once, every other link accepted
// by its owner before anything is read through it.
// E: bool link_ok(link) for a link >= 2; void links(link, validw, next) for link 1 or an accepted link >= 2.
// on_entry(pos, link, validw): entry number `pos` of the chain; false stops the walk.  Returns whether the end was reached.
template <class E, class F>
SI_HD static inline bool si_chain_walk(uint32_t head, const E &e, F &&on_entry) {
  uint32_t link = head;
  bool inl = false;
  for (uint32_t pos = 0; link != KV_NULL; pos++) {
    if (pos >= KV_MAX_CHAIN) return false;
    if (link == KV_INLINE) {
      if (inl) return false;
      inl = true;
    } else if (!e.link_ok(link)) {
      return false;
    }
    uint32_t validw, next;
    e.links(link, validw, next);
    if (!on_entry(pos, link, validw)) return false;
    link = next;
  }
  return true;
}
// ... as the image sees it.  on_ovf(m, link): the m-th overflow entry of the chain; false stops the walk.
struct si_walk {
  uint32_t count;    // overflow entries visited
  uint32_t before;   // ... of them ahead of the inline entry
  uint32_t rows;     // valid slots of the visited entries
  uint32_t linked;   // the inline entry is part of the chain
  uint32_t ok;       // the walk reached the end of the chain
};
template <class E, class F>
SI_HD static inline si_walk si_walk_chain(uint32_t head, const E &e, F &&on_ovf) {
  si_walk w = {0, 0, 0, 0, 1};
  w.ok = si_chain_walk(head, e, [&](uint32_t, uint32_t link, uint32_t validw) {
    if (link == KV_INLINE) {
      w.linked = 1;
      w.before = w.count;
    } else {
      if (!on_ovf(w.count, link)) return false;
      w.count++;
    }
    w.rows += si_valid_count(validw);
    return true;
  });
  return w;
}

// ---- the per-entry check ------------------------------------------------------------------------------------------------
struct si_geom {
  uint64_t global_size, n_buckets, n_overflow;
  uint32_t src_index, src_count, dst_index, dst_count;
};
SI_HD static inline uint32_t si_check_id(uint64_t id, bool has_prev, uint64_t prev_id, const si_geom &g) {
  uint32_t bad = 0;
  if (has_prev && prev_id >= id) bad |= SI_BAD_ORDER;
  if (id >= g.global_size) bad |= SI_BAD_RANGE;
  if (id % g.dst_count != g.dst_index || id % g.src_count != g.src_index) bad |= SI_BAD_HOME;
  return bad;
}
// a lock table's slot b.  A: si_dir dir(b)
template <class A>
SI_HD static inline uint32_t si_check_slot(const A &a, uint64_t b, const si_geom &g) {
  const si_dir d = a.dir(b);
  return si_check_id(d.id, b > 0, b > 0 ? a.dir(b - 1).id : 0, g);
}
// bucket b of a kv table.  A: si_dir dir(b); void inline_links(b, validw, next, head); void ovf_links(x, validw, next)
// (x < n_overflow: never called with another); for the table report also void keys(b, link, k[4]).
// The bucket's chain as si_chain_walk and state_stats.h st_bucket_walk take it: a link is good inside the bucket's own run,
// and *bad records one that is not.
template <class A>
struct si_image_chain {
  const A &a;
  uint64_t b;
  si_dir d;
  uint32_t *bad;
  SI_HD inline uint32_t head() const {
    uint32_t validw, next, head;
    a.inline_links(b, validw, next, head);
    return head;
  }
  SI_HD inline bool link_ok(uint32_t link) const {
    const uint64_t x = (uint64_t)link - 2u;
    if (x >= d.first && x < (uint64_t)d.first + d.count) return true;
    *bad |= SI_BAD_LINK;
    return false;
  }
  SI_HD inline void links(uint32_t link, uint32_t &validw, uint32_t &next) const {
    uint32_t head;
    if (link == KV_INLINE) a.inline_links(b, validw, next, head);
    else a.ovf_links((uint64_t)link - 2u, validw, next);
  }
  SI_HD inline void keys(uint32_t link, uint64_t k[4]) const { a.keys(b, link, k); }
};
// *rows += the valid slots of the bucket's chain.
template <class A>
SI_HD static inline uint32_t si_check_bucket(const A &a, uint64_t b, const si_geom &g, uint64_t *rows) {
  const si_dir d = a.dir(b);
  si_dir p = {0, 0, 0};
  if (b > 0) p = a.dir(b - 1);
  uint32_t bad = si_check_id(d.id, b > 0, p.id, g);
  const uint64_t want = b > 0 ? (uint64_t)p.first + p.count : 0, end = (uint64_t)d.first + d.count;
  if (d.first != want || d.count > SI_MAX_RUN || end > g.n_overflow || (b + 1 == g.n_buckets && end != g.n_overflow)) bad |= SI_BAD_RUN;
  if (bad & SI_BAD_RUN) return bad;  // (no link can be judged, and none is followed)
  uint32_t validw, next, head;
  a.inline_links(b, validw, next, head);
  const si_image_chain<A> ch = {a, b, d, &bad};
  const si_walk w = si_walk_chain(head, ch, [&](uint32_t m, uint32_t link) {
    if ((uint64_t)link - 2u == (uint64_t)d.first + m) return true;
    bad |= SI_BAD_CHAIN;
    return false;
  });
  if (!(bad & (SI_BAD_LINK | SI_BAD_CHAIN)) && (!w.ok || w.count != d.count)) bad |= SI_BAD_CHAIN;
  if (!w.linked) {
    if (validw) bad |= SI_BAD_UNLINKED;
    if (next >= 2u) (void)ch.link_ok(next);  // (never followed, but import rewrites it: 0, 1 or inside the run like every link)
  }
  *rows += w.rows;
  return bad;
}

// ---- an image in host memory ---------------------------------------------------------------------------------------------
static inline uint32_t si_ld32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
static inline uint64_t si_ld64(const uint8_t *p) { uint64_t v; memcpy(&v, p, 8); return v; }
// table t's section of an image whose header h has passed si_header_check: the A of si_check_slot / si_check_bucket /
// si_image_chain over plain bytes at any alignment
struct si_host_image {
  const uint8_t *p_dir, *p_inl, *p_ovf;
  uint32_t stride;
  si_host_image(const si_header &h, uint32_t t, const uint8_t *image, bool lock)
      : p_dir(image + h.table[t].offset), p_inl(p_dir + 16 * h.table[t].n_buckets),
        p_ovf(lock ? p_inl : p_inl + h.table[t].n_buckets * h.stride), stride(h.stride) {}
  const uint8_t *entry(uint64_t b, uint32_t link) const { return link == KV_INLINE ? p_inl + b * stride : p_ovf + (uint64_t)(link - 2u) * stride; }
  si_dir dir(uint64_t b) const { return si_dir{si_ld64(p_dir + 16 * b), si_ld32(p_dir + 16 * b + 8), si_ld32(p_dir + 16 * b + 12)}; }
  void inline_links(uint64_t b, uint32_t &validw, uint32_t &next, uint32_t &head) const {
    const uint8_t *e = entry(b, KV_INLINE);
    validw = si_ld32(e + KV_VALID_OFF); next = si_ld32(e + offsetof(kv_hdr, next)); head = si_ld32(e + offsetof(kv_hdr, head));
  }
  void ovf_links(uint64_t x, uint32_t &validw, uint32_t &next) const {
    const uint8_t *e = p_ovf + x * stride;
    validw = si_ld32(e + KV_VALID_OFF); next = si_ld32(e + offsetof(kv_hdr, next));
  }
  void keys(uint64_t b, uint32_t link, uint64_t k[4]) const {
    const uint8_t *e = entry(b, link);
    for (uint32_t i = 0; i < 4; i++) k[i] = si_ld64(e + 8 * i);
  }
};
