// state_block.h -- the tables of an engine cut into blocks of buckets, so that two replicas on different devices can find the
// few places where they differ and ship only those: one source for the kernels (k_block.hip: dint_state_block_digest /
// dint_state_block_select / dint_state_block_rows / dint_state_block_diff, include/dint_abi.h) and the host forms over
// caller-provided memory (dint_state_block_digest_host / _rows_host / _diff_host, include/dint_driver.h), as state_sync.h is
// for the state sync and state_compact.h for the compaction.  Integer arithmetic only.
//
// A BLOCK is B consecutive LOCAL buckets of one table: B a power of two, BK_MIN_BUCKETS <= B <= BK_MAX_BUCKETS; the last
// block of a table may be short.  Block ids are u32 and run over the tables in table order: table 0's blocks, then table
// 1's ...  Two engines of one workload, n_rows, shard and B have the same geometry, and a key has the same block in both.
//
//   digest  per block {rows, sum, xr, 0} (state_sync.h ss_digest) over every valid slot of the chains of its buckets --
//           shadowed duplicates included, as dint_state_digest counts them: on sound tables the blocks of a table merge to
//           the table's digest
//   rows    the VISIBLE rows of a block (per key the first valid slot in chain order) as canonical 64-byte records
//           (is_del = 0), ascending bucket, chain order
//   diff    state_sync.h ss_bucket_diff per bucket, side a = the bucket's RUN of such records in a row list (bk_run below),
//           side b = the replica's chain
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "state_rehash.h"
#include "state_sync.h"

#define BK_MIN_BUCKETS 64u
#define BK_MAX_BUCKETS (1u << 20)
#define BK_CHUNK 64u                      // the digest's unit of work: a wave's buckets; a block is a whole number of them
#define BK_MAX_TABLES 5u
#define BK_MAX_RUN (4u * KV_MAX_CHAIN)    // rows of one bucket in a row list at most: what a chain can hold visible
#define BK_MAX_ROWS 0xFFFFFFF0ull         // rows of a row list at most (a run's start is a u32)

// what the checks found (a bit each)
enum : uint32_t {
  BK_BAD_IDS = 1u,    // ids not strictly ascending, or one out of range
  BK_BAD_TABLE = 2u,  // a row of a table the workload has not, or a delete record
  BK_BAD_HOME = 4u,   // a row that is home to another shard or to a block that is not listed
  BK_BAD_ORDER = 8u,  // (table, bucket) decreasing
  BK_BAD_RUN = 16u    // more than BK_MAX_RUN rows of one bucket
};
SS_HD static inline const char *bk_bad_name(uint32_t bad) {
  if (bad & BK_BAD_IDS) return "block ids must be strictly ascending and in range";
  if (bad & BK_BAD_TABLE) return "a row names a table the workload has not, or is a delete record";
  if (bad & BK_BAD_HOME) return "a row is not home to a bucket of a listed block";
  if (bad & BK_BAD_ORDER) return "the rows are not grouped by (table, bucket) ascending";
  if (bad & BK_BAD_RUN) return "more rows of one bucket than a chain can hold";
  return "nothing";
}

SS_HD static inline bool bk_valid_buckets(uint64_t B) { return B >= BK_MIN_BUCKETS && B <= BK_MAX_BUCKETS && (B & (B - 1)) == 0; }
SS_HD static inline uint32_t bk_log2(uint32_t B) {
  uint32_t s = 0;
  while ((1u << s) < B) s++;
  return s;
}

// ---- the geometry --------------------------------------------------------------------------------------------------------
struct bk_geom {
  uint32_t n_tables, shift;           // B = 1 << shift
  uint32_t first[BK_MAX_TABLES + 1];  // table t's blocks are ids [first[t], first[t + 1]); first[n_tables] = all blocks
  uint64_t n_local[BK_MAX_TABLES];
};
struct bk_block {
  uint32_t table;
  uint64_t first, count;  // local buckets [first, first + count)
};
SS_HD static inline uint64_t bk_table_blocks(uint64_t n_local, uint32_t shift) { return (n_local + ((1ull << shift) - 1)) >> shift; }
// false: B is not a block size, or the ids do not fit a u32
SS_HD static inline bool bk_geom_make(bk_geom &g, uint32_t n_tables, const uint64_t *n_local, uint64_t B) {
  if (!bk_valid_buckets(B) || n_tables == 0 || n_tables > BK_MAX_TABLES) return false;
  g.n_tables = n_tables;
  g.shift = bk_log2((uint32_t)B);
  uint64_t at = 0;
  for (uint32_t t = 0; t < BK_MAX_TABLES; t++) {
    g.first[t] = (uint32_t)at;
    g.n_local[t] = t < n_tables ? n_local[t] : 0;
    at += bk_table_blocks(g.n_local[t], g.shift);
    if (at > 0xFFFFFFF0ull) return false;
  }
  g.first[BK_MAX_TABLES] = (uint32_t)at;
  for (uint32_t t = n_tables; t < BK_MAX_TABLES; t++) g.first[t] = (uint32_t)at;
  return true;
}
SS_HD static inline uint32_t bk_blocks(const bk_geom &g) { return g.first[g.n_tables]; }
// id < bk_blocks(g)
SS_HD static inline bk_block bk_locate(const bk_geom &g, uint32_t id) {
  uint32_t t = 0;
  while (t + 1 < g.n_tables && id >= g.first[t + 1]) t++;
  bk_block b;
  b.table = t;
  b.first = (uint64_t)(id - g.first[t]) << g.shift;
  const uint64_t left = g.n_local[t] - b.first;
  b.count = left < (1ull << g.shift) ? left : (1ull << g.shift);
  return b;
}
// table < n_tables, bucket < n_local[table]
SS_HD static inline uint32_t bk_id_of(const bk_geom &g, uint32_t table, uint64_t bucket) { return g.first[table] + (uint32_t)(bucket >> g.shift); }
// the digest's chunks: BK_CHUNK buckets each, numbered like the blocks of B = BK_CHUNK
SS_HD static inline uint64_t bk_table_chunks(uint64_t n_local) { return (n_local + BK_CHUNK - 1) / BK_CHUNK; }

// where id sits in ids[0 .. n) (ascending), or n
template <class Ids>
SS_HD static inline uint32_t bk_find_id(const Ids &ids, uint32_t n, uint32_t id) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {  // (bounded by 32 rounds whatever ids holds)
    const uint32_t mid = lo + (hi - lo) / 2;
    if (ids[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && ids[lo] == id ? lo : n;
}

// ---- one row of a row list -------------------------------------------------------------------------------------------------
// the home of record r in an engine of this geometry: place = table << 56 | local bucket (the order a list must come in).
// LD: the loads (u32(p), u64(p)) -- plain ones on the device, where a list is 8-byte aligned; memcpy on the host.
struct bk_place {
  uint32_t bad;    // BK_BAD_TABLE / BK_BAD_HOME, or 0
  uint32_t table;
  uint64_t bucket;
  SS_HD inline uint64_t order() const { return ((uint64_t)table << 56) | bucket; }
};
// global(key, table) = the key's GLOBAL bucket: fasthash64(key) % the table's hash size
template <class LD, class Global>
SS_HD static inline bk_place bk_row_place(const uint8_t *r, const bk_geom &g, uint32_t shard_index, uint32_t shard_count, Global &&global) {
  bk_place p = {0, 0, 0};
  const uint32_t w13 = LD::u32(r + offsetof(LrRecord, is_del));
  p.table = (w13 >> 8) & 0xFFu;
  if (p.table >= g.n_tables || (w13 & 0xFFu)) {
    p.bad = BK_BAD_TABLE;
    return p;
  }
  p.bucket = sr_local_bucket(global(LD::u64(r), p.table), shard_index, shard_count);
  if (p.bucket >= g.n_local[p.table]) p.bad = BK_BAD_HOME;  // (SR_FOREIGN is beyond every table)
  return p;
}

// ---- a bucket's run of a row list as state_sync.h's "row list" -------------------------------------------------------------------
// records [0, n) at rec, in list order; a key that appears twice: the first is the visible one, as find has it
template <class LD>
struct bk_run {
  const uint8_t *rec;
  uint32_t n;
  SS_HD inline uint32_t begin() const { return 0; }
  SS_HD inline uint32_t next(uint32_t p) const { return p + 1; }
  SS_HD inline bool ok(uint32_t p) const { return p < n; }
  SS_HD inline bool same(uint32_t p, uint32_t q) const { return p == q; }
  SS_HD inline uint64_t key(uint32_t p) const { return LD::u64(rec + (size_t)p * 64); }
  SS_HD inline uint32_t ver(uint32_t p) const { return LD::u32(rec + (size_t)p * 64 + offsetof(LrRecord, ver)); }
  SS_HD inline uint32_t val32(uint32_t p, uint32_t w) const { return LD::u32(rec + (size_t)p * 64 + offsetof(LrRecord, val) + 4 * w); }
  SS_HD inline uint32_t find(uint64_t k) const {
    for (uint32_t p = 0; p < n; p++)
      if (key(p) == k) return p;
    return n;
  }
};
static_assert(offsetof(LrRecord, val) == 8 && offsetof(LrRecord, key) == 0, "a row list holds canonical log records");
