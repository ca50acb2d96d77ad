// state_rehash.h -- the layout rule of a rehash: the rows of a set of source engines placed into a BLANK destination of
// another bucket count (and shard), one source for the kernels (k_rehash.hip: dint_state_rehash, include/dint_abi.h) and the
// host form (dint_state_rehash_place_host, include/dint_driver.h), as state_image.h is for the state image.
//
// SOURCE ORDER of a row: (position of its engine in srcs, local bucket, position of its entry in the chain, slot),
// ascending -- dint_dump_rows order, engine after engine.  Every valid slot counts, shadowed duplicates included.
//
// A row is HOME to the destination (hash size S', shard j of H) when g' = fasthash64(key) % S' has g' % H == j; its
// destination bucket is local bucket g' / H.  For each destination bucket the k rows that land in it, taken in source
// order, are row r = 0 .. k - 1:
//   the chain has ceil(k / 4) entries; chain position r / 4, slot r % 4, holds row r: no holes
//   chain position 0 is the INLINE entry (head = 1): a bucket of at most four rows costs one sector per probe
//   chain position x >= 1 of local bucket b is pool entry base[b] + x - 1, base = the exclusive scan, over local buckets
//   ascending, of the buckets' overflow counts, starting at pool_top (0: the destination is blank); ONE bump of pool_top
//   per table, free and pend lists stay empty
//   key, version and value are copied verbatim; a valid byte is 1; unused slots, lock bytes, smallbank counters and owner
//   keys are zero; an empty bucket is not written
// Two rows of one key share their source bucket and their destination bucket, so they keep their order: the visible row
// of every key stays its visible row.
//
// In the stable order by destination bucket, the scan over ROWS of "this row opens an overflow entry" is that entry's pool
// index: the buckets are ascending there, and inside a bucket so are the entries.  Kernels and host form both use it, so
// no per-bucket array is needed.  Integer arithmetic only.
#pragma once
#include <stdint.h>

#include "dint_kv_core.h"

#if defined(__HIPCC__)
#define SR_HD __host__ __device__
#else
#define SR_HD
#endif

#define SR_FOREIGN 0xFFFFFFFFFFFFFFFFull  // "no local bucket": the row is home to another shard
#define SR_MAX_SRCS 255u                  // engines one call reads (a shard set has at most 255)
#define SR_MAX_ROWS 0xFFFFFFF0ull         // rows of one table over all sources: positions are 32-bit

// ---- where a row goes ---------------------------------------------------------------------------------------------------
// g = hash % hash_size (the caller's modulus); the local bucket, or SR_FOREIGN
SR_HD static inline uint64_t sr_local_bucket(uint64_t g, uint32_t shard_index, uint32_t shard_count) {
  if (shard_count <= 1) return g;
  return g % shard_count == shard_index ? g / shard_count : SR_FOREIGN;
}
// row r of its bucket
SR_HD static inline uint32_t sr_chain_pos(uint32_t r) { return r >> 2; }
SR_HD static inline uint32_t sr_slot(uint32_t r) { return r & 3u; }
SR_HD static inline bool sr_opens_entry(uint32_t r) { return (r & 3u) == 0; }
SR_HD static inline bool sr_opens_overflow(uint32_t r) { return r >= 4u && (r & 3u) == 0; }
// entries / overflow entries of a bucket of k rows
SR_HD static inline uint32_t sr_entries(uint32_t k) { return (k + 3u) >> 2; }
SR_HD static inline uint32_t sr_overflow(uint32_t k) { return k > 4u ? sr_entries(k) - 1u : 0u; }
// the link of chain position x whose pool entry (x >= 1) is `pool`
SR_HD static inline uint32_t sr_link(uint32_t x, uint32_t pool) { return x == 0 ? KV_INLINE : pool + 2u; }
// valid bytes of an entry that holds m rows (1 .. 4) in slots 0 .. m - 1
SR_HD static inline uint32_t sr_validw(uint32_t m) { return 0x01010101u >> (8u * (4u - m)); }

// ---- the locator of a source row: {source number : 16, entry index in the source's entries[] : 46, slot : 2} ---------------
SR_HD static inline uint64_t sr_loc(uint32_t src, uint64_t entry, uint32_t slot) { return (uint64_t)src << 48 | entry << 2 | slot; }
SR_HD static inline uint32_t sr_loc_src(uint64_t loc) { return (uint32_t)(loc >> 48); }
SR_HD static inline uint64_t sr_loc_entry(uint64_t loc) { return (loc >> 2) & ((1ull << 46) - 1); }
SR_HD static inline uint32_t sr_loc_slot(uint64_t loc) { return (uint32_t)loc & 3u; }

// key bits the sort looks at: the local buckets 0 .. n_local - 1 and n_local itself, the key of a foreign row
SR_HD static inline uint32_t sr_key_bits(uint64_t n_local) {
  uint32_t b = 1;
  while (b < 32u && (n_local >> b) != 0) b++;
  return b;
}
