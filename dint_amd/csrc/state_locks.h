// state_locks.h -- which lock units of a server are held, who may sit on them, and which records may release them: one source for
// the kernels (k_locks_state.hip: dint_state_locks / dint_state_unlock, include/dint_abi.h) and the host forms over a state image and
// over a record list (dint_state_locks_image_host / dint_state_unlock_check_host, include/dint_driver.h), as state_stats.h is for the
// table report.  Integer arithmetic only.
//
//   workload    unit                                                   held iff            a, b (as dint_read_locks)
//   lock_fasst  d_lock_tbl[local slot] = {lock, ver}                   lock != 0           lock, ver   (a version alone holds nothing)
//   lock_2pl    d_lock_tbl[local slot] = {num_ex, num_sh}              either non-zero     num_ex, num_sh
//   tatp        byte q of the inline header's word at KV_LOCKB_OFF     byte non-zero       byte, 0
//   smallbank   pair q at KV_SB_LOCK_OFF of the inline entry           either non-zero     num_ex, num_sh
// (tatp / smallbank: state_image.h si_locks_held counts the same units.)
//
// A unit's LOCAL slot is dint_read_locks' index: lock tables global slot / shard_count; kv q * n_local + local bucket.  The ORDER
// of a list is ascending table, then ascending local bucket, then ascending q (lock tables: ascending local slot): bucket-major, so
// that one header read serves a bucket's four units.
//
// CANDIDATES (kv).  The lock slot of a key is fasthash64(key) % (4 * hash_size) = q * hash_size + global bucket, and the rows of
// such a key live in that bucket's chain.  cand_rows = the valid slots of the chain whose key's lock slot is the unit (shadowed
// duplicates count, holes do not); the walk is state_image.h si_chain_walk: KV_MAX_CHAIN entries at most, every link judged by its
// owner before anything is read through it.  A walk that does not reach the chain's end sets LK_WALK_CUT and reports what it saw.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/dint_abi.h"
#include "dint_device.h"
#include "dint_kv_core.h"
#include "state_image.h"

static_assert(sizeof(dint_lock_record) == 32 && offsetof(dint_lock_record, key) == 16 && offsetof(dint_lock_record, cand_rows) == 24 &&
              offsetof(dint_lock_record, table) == 28 && offsetof(dint_lock_record, flags) == 29, "a lock record is four 8-byte words");
static_assert(sizeof(dint_lock_stats) == 128 && sizeof(dint_unlock_stats) == 128, "sixteen words each");

enum : uint32_t { LK_NONE = 0, LK_FASST = 1, LK_2PL = 2, LK_TATP = 3, LK_SMALLBANK = 4 };
#define LK_KEY_OWNER DINT_LOCK_KEY_OWNER
#define LK_KEY_ROW DINT_LOCK_KEY_ROW
#define LK_WALK_CUT DINT_LOCK_WALK_CUT
#define LK_MAX_TABLES 5u
#define LK_MAX_LIST 0xFFFFFFF0ull    // records of a list: fewer than this
#define LK_NO_INDEX 0xFFFFFFFFFFFFFFFFull

SI_HD static inline uint32_t lk_mode(uint32_t workload) {
  return workload == DINT_WL_FASST ? LK_FASST : workload == DINT_WL_2PL ? LK_2PL : workload == DINT_WL_TATP ? LK_TATP :
         workload == DINT_WL_SMALLBANK ? LK_SMALLBANK : LK_NONE;
}
SI_HD static inline bool lk_is_kv(uint32_t mode) { return mode == LK_TATP || mode == LK_SMALLBANK; }
SI_HD static inline bool lk_held(uint32_t mode, uint32_t a, uint32_t b) { return mode == LK_FASST ? a != 0 : (a | b) != 0; }
// does the unit's current {a, b} equal a record's?  (lock_fasst: the version moves independently of the lock)
SI_HD static inline bool lk_same(uint32_t mode, uint32_t a, uint32_t b, uint32_t ra, uint32_t rb) {
  return a == ra && (mode == LK_FASST || b == rb);
}

// the lock units of one engine (or of the source of an image)
struct lk_geom {
  uint32_t mode, n_tables, shard_index, shard_count, same_key;
  uint64_t n_local[LK_MAX_TABLES];  // local buckets (kv) / local slots (lock tables)
  uint64_t size[LK_MAX_TABLES];     // the table's global bucket count / n_slots
};
SI_HD static inline uint64_t lk_n_local(uint64_t size, uint32_t shard_count) { return (size + shard_count - 1) / shard_count; }

// where a record's unit lies; ok = the record names a unit this engine has.  ord = the unit's place in a table's order.
struct lk_unit {
  bool ok;
  uint64_t bucket;  // local bucket / local slot
  uint32_t q;
  uint64_t ord;
};
SI_HD static inline lk_unit lk_unit_of(const lk_geom &g, uint32_t table, uint64_t slot) {
  lk_unit u = {false, 0, 0, 0};
  if (table >= g.n_tables || table >= LK_MAX_TABLES) return u;  // (the table is range-checked before it indexes anything)
  const uint64_t nl = g.n_local[table];
  if (!lk_is_kv(g.mode)) {
    if (slot >= nl) return u;
    u.ok = true; u.bucket = slot; u.ord = slot;
    return u;
  }
  if (nl == 0 || slot / nl >= 4) return u;
  u.q = (uint32_t)(slot / nl);
  u.bucket = slot - (uint64_t)u.q * nl;
  if (u.bucket * g.shard_count + g.shard_index >= g.size[table]) return u;  // a sharded engine's last local bucket beyond the table
  u.ok = true;
  u.ord = u.bucket * 4 + u.q;
  return u;
}
// the list check of one record: r, and p = the record before it (has_prev).  true = the list is refused at r.
SI_HD static inline bool lk_record_bad(const lk_geom &g, const dint_lock_record &r, bool has_prev, const dint_lock_record &p) {
  const lk_unit u = lk_unit_of(g, r.table, r.slot);
  if (!u.ok || !lk_held(g.mode, r.a, r.b)) return true;
  if (has_prev) {
    const lk_unit v = lk_unit_of(g, p.table, p.slot);
    if (v.ok && (p.table > r.table || (p.table == r.table && v.ord >= u.ord))) return true;  // (v not ok: the list is refused at p already)
  }
  return false;
}

// ---- candidates ------------------------------------------------------------------------------------------------------------------
struct lk_cand {
  uint32_t rows, flags;  // LK_KEY_ROW | LK_WALK_CUT
  uint64_t key;
};
// E: state_image.h si_chain_walk's accessor with keys(link, k[4]) (state_dev.h sd_bucket, state_image.h si_image_chain);
// lock_hash = q * hash_size + global bucket of the unit, lockmod = % (4 * hash_size)
template <class E>
SI_HD static inline lk_cand lk_candidates(const E &ch, uint32_t head, dint_mod lockmod, uint64_t lock_hash) {
  lk_cand c = {0, 0, 0};
  const bool ok = si_chain_walk(head, ch, [&](uint32_t, uint32_t link, uint32_t validw) {
    if (!validw) return true;
    uint64_t k[4];
    ch.keys(link, k);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < 4; i++)
      if (((validw >> (8 * i)) & 0xFFu) && dint_fastmod(dint_hash_key(k[i]), lockmod) == lock_hash) {
        if (!c.rows) c.key = k[i];
        c.rows++;
      }
    return true;
  });
  if (c.rows) c.flags |= LK_KEY_ROW;
  if (!ok) c.flags |= LK_WALK_CUT;
  return c;
}

// the record of a held unit (owner: tatp with DINT_FLAG_LOCK_SAME_KEY, the key at KV_OWNER_OFF + 8 q; c: kv only)
SI_HD static inline dint_lock_record lk_record(uint32_t table, uint64_t slot, uint32_t a, uint32_t b, bool has_owner, uint64_t owner,
                                               const lk_cand &c) {
  dint_lock_record r;
  r.slot = slot; r.a = a; r.b = b;
  r.cand_rows = c.rows;
  r.table = (uint8_t)table;
  r.zero = 0;
  if (has_owner) {
    r.key = owner;
    r.flags = (uint8_t)(LK_KEY_OWNER | (c.flags & LK_WALK_CUT));
  } else {
    r.key = c.rows ? c.key : 0;
    r.flags = (uint8_t)c.flags;
  }
  return r;
}
// r as the four 8-byte words it is stored as
SI_HD static inline void lk_record_words(const dint_lock_record &r, uint64_t w[4]) {
  w[0] = r.slot;
  w[1] = (uint64_t)r.a | ((uint64_t)r.b << 32);
  w[2] = r.key;
  w[3] = (uint64_t)r.cand_rows | ((uint64_t)r.table << 32) | ((uint64_t)r.flags << 40) | ((uint64_t)r.zero << 48);
}
SI_HD static inline dint_lock_record lk_record_of_words(const uint64_t w[4]) {
  dint_lock_record r;
  r.slot = w[0]; r.a = (uint32_t)w[1]; r.b = (uint32_t)(w[1] >> 32); r.key = w[2];
  r.cand_rows = (uint32_t)w[3]; r.table = (uint8_t)(w[3] >> 32); r.flags = (uint8_t)(w[3] >> 40); r.zero = (uint16_t)(w[3] >> 48);
  return r;
}

// ---- the statistics: the words a workgroup's partial holds (LK_PART of them), summed per range of workgroups ---------------------
#define LK_PART 8u
enum : uint32_t { LKS_HELD = 0, LKS_SUM_A, LKS_SUM_B, LKS_NO_ROW, LKS_WALK_CUT };          // the listing and the sweep (held = released)
enum : uint32_t { LKU_TABLE = 0, LKU_STALE = 5, LKU_REL_A = 6, LKU_REL_B = 7 };            // the list form of the release
