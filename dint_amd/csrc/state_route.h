// state_route.h -- where a canonical 64-byte record (log_replay.h LrRecord: a drained log record, a dint_state_diff record, a
// dint_state_block_rows row) belongs in a set of H shards, one source for the kernels (k_rroute.hip: dint_records_route,
// include/dint_abi.h), the host form over caller-provided memory (dint_records_route_host, include/dint_driver.h) and the
// consumers that take a shard (k_state.hip the repair, k_fold.hip the fold, k_replay.hip the replay's check), as state_block.h is
// for the block sync.  Integer arithmetic only.
//
//   global bucket  g = fasthash64(key) % hash_size[table]           (dint_device.h dint_hash_key, dint_fastmod)
//   home           g % H: the one shard j of H for which state_rehash.h sr_local_bucket(g, j, H) is not SR_FOREIGN
//   local bucket   g / H in that shard
// A record whose table the workload has not has NO HOME: nothing is concluded from its key.
//
// ROUTE: the stable partition of a list by home.  Shard 0's records in their input order, then shard 1's ...; offsets[h] =
// records of the shards below h, offsets[H] = n.  A list that is ascending in (table, g) -- dint_state_diff's order on an unsharded
// engine -- leaves every piece ascending in (table, g / H): g ascending with g % H fixed gives g / H non-decreasing, which is the
// order shard h's dint_state_repair takes.  A log keeps its order per row: a row has one home.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "dint_device.h"
#include "log_replay.h"
#include "state_rehash.h"

#define RR_MAX_SHARDS 255u      // shards of a destination layout at most (a home fits a byte; SR_MAX_SRCS)
#define RR_MAX_TABLES 5u
#define RR_TILE 512u            // records per workgroup of the count and the write stage (32 KB of LDS staging)
#define RR_NO_HOME 0xFFFFFFFFu
#define RR_NO_INDEX 0xFFFFFFFFFFFFFFFFull  // "no record without a home"

static_assert(offsetof(LrRecord, key) == 0 && offsetof(LrRecord, is_del) == 52 && offsetof(LrRecord, table) == 53, "record layout");

struct rr_geom {
  uint32_t n_tables, n_shards;      // n_shards >= 1
  dint_mod mod[RR_MAX_TABLES];      // % hash_size[table]
};
// w13 = the record's 32-bit word at byte 52 {is_del, table, pad, pad}
SR_HD static inline uint32_t rr_word_table(uint32_t w13) { return (w13 >> 8) & 0xFFu; }
// the global bucket of a key of `table` (table < n_tables)
SR_HD static inline uint64_t rr_global(uint64_t key, uint32_t table, const dint_mod *mod) { return dint_fastmod(dint_hash_key(key), mod[table]); }
// the home of global bucket g among H shards: the j with sr_local_bucket(g, j, H) == g / H
SR_HD static inline uint32_t rr_home_of(uint64_t g, uint32_t H) { return H <= 1 ? 0u : (uint32_t)(g % H); }
// the home of a record, or RR_NO_HOME.  The table is range-checked before it indexes anything.
SR_HD static inline uint32_t rr_home(uint64_t key, uint32_t table, const rr_geom &g) {
  if (table >= g.n_tables) return RR_NO_HOME;
  return rr_home_of(rr_global(key, table, g.mod), g.n_shards);
}
// the local bucket of a record in shard (index, count), SR_FOREIGN when it is home to another shard (table < n_tables)
SR_HD static inline uint64_t rr_local(uint64_t key, uint32_t table, const dint_mod *mod, uint32_t shard_index, uint32_t shard_count) {
  return sr_local_bucket(rr_global(key, table, mod), shard_index, shard_count);
}

// tiles of a list, and the words of the count stage's scratch (shard-major: [shard][tile])
SR_HD static inline uint64_t rr_tiles(uint64_t n) { return (n + RR_TILE - 1) / RR_TILE; }
#define RR_MAX_COUNTS 0xFFFFFFF0ull  // (shards x tiles: the scan's length is a u32)
