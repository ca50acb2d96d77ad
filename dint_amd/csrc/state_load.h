// state_load.h -- the rule of a bulk load: where rows given in INSERTION ORDER land in a table that holds nothing, and which rows
// the reference's population has.  One source for the kernels (k_load.hip: dint_load_rows_device, dint_populate_device,
// include/dint_abi.h) and the host forms (dint_state_load_place_host, dint_populate_rows_host, include/dint_driver.h), as
// state_rehash.h is for the rehash.  Integer arithmetic only.
//
// PLACEMENT.  Rows i = 0 .. n - 1.  A row is HOME when g = fasthash64(key) % hash_size has g % shard_count == shard_index; its
// bucket is local bucket g / shard_count (state_rehash.h sr_local_bucket).  Rows home to another shard are skipped and counted.
// The k home rows of a bucket, in insertion order r = 0 .. k - 1, lie as kvs_insert into an empty bucket leaves them
// (dint_kv_core.h kv_apply, KV_ACT_INS: first invalid slot in chain order, else a new entry PREPENDED):
//   entry x = r / 4, slot r % 4, no holes; entry 0 is the inline entry, entry x >= 1 a pool entry
//   the chain runs newest entry first: head = link of entry ceil(k / 4) - 1, next of entry x = link of entry x - 1, next of the
//   inline entry = 0
//   version = vers[i] (0 without vers), valid byte 1, value verbatim; lock bytes, owner keys, smallbank counters are not written
//   pool indices = the exclusive scan, in stable (bucket, i) order, of "this row opens an overflow entry", from 0; pool_top takes
//   one store per table, free and pend lists stay empty
// Duplicate keys are rows like any other (kvs_insert does not look).  The visible row of a key is the first in chain order:
// the earliest row of the NEWEST entry that holds the key.
// (state_rehash.h places inline-entry-first, oldest first: the same rows, another chain order.)
//
// GENERATION.  The rows of subscriber / account s of a table group are a function of s and the fastrand state at s's first draw
// (sl_gen_sub).  Draws per subscriber: store 12, tatp SUBSCRIBER 17, SECONDARY SUBSCRIBER and smallbank none -- the state at s
// is sl_lcg_jump(seed, draws * s).  ACCESS INFO and SPECIAL FACILITY + CALL FORWARDING draw a data-dependent number
// (sl_pick_types rejects): the state at the start of every tile of SL_TILE subscribers comes from running sl_gen_sub with an
// emitter that counts (sl_tile_walk) -- a prefix property of the group, not of n.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "state_rehash.h"

#define SL_HD SR_HD

#define SL_MAX_ROWS SR_MAX_ROWS  // rows of one call: positions are 32-bit
#define SL_TILE 256u             // subscribers per workgroup of the generation kernels, and per entry of the tile table

// ---- placement -----------------------------------------------------------------------------------------------------------
// next of chain position x (x >= 1: `prev_pool` = the pool index of entry x - 1, read only for x >= 2)
SL_HD static inline uint32_t sl_next(uint32_t x, uint32_t prev_pool) { return x == 0 ? KV_NULL : sr_link(x - 1u, prev_pool); }
// a bucket of k rows is refused when its chain would be longer than a walk goes (dint_kv_core.h KV_MAX_CHAIN)
SL_HD static inline bool sl_chain_too_long(uint32_t entries) { return entries > KV_MAX_CHAIN; }

// ---- fastrand (tatp/udp/tatp.h:32-35) and its jump --------------------------------------------------------------------------
#define SL_LCG_A 1103515245ull
#define SL_LCG_C 12345ull
#define SL_SEED 0xdeadbeefull
SL_HD static inline uint32_t sl_lcg_next(uint64_t &s) {
  s = s * SL_LCG_A + SL_LCG_C;
  return (uint32_t)(s >> 32);
}
// the state k draws after s: the k-fold composition of x -> A x + C, by square and multiply (mod 2^64 throughout)
SL_HD static inline uint64_t sl_lcg_jump(uint64_t s, uint64_t k) {
  uint64_t a = SL_LCG_A, c = SL_LCG_C, ra = 1, rc = 0;
  for (; k; k >>= 1) {
    if (k & 1) {
      ra = a * ra;
      rc = a * rc + c;
    }
    c = (a + 1) * c;
    a = a * a;
  }
  return ra * s + rc;
}

// ---- the population's table groups -------------------------------------------------------------------------------------------
// A group is generated from one fastrand stream; it fills one table, or two (tatp SPECIAL FACILITY + CALL FORWARDING: `which`
// 0 / 1 in an emitter's call).  DINT_WL_* are include/dint_abi.h's: store 3, tatp 4, smallbank 5.
enum : uint32_t { SL_G_STORE = 0, SL_G_SB_SAV, SL_G_SB_CHK, SL_G_SUB, SL_G_SEC, SL_G_AI, SL_G_SFCF, SL_G_NONE };
#define SL_WL_STORE 3u
#define SL_WL_TATP 4u
#define SL_WL_SMALLBANK 5u
// the group that fills `table`, and which of its tables that is
SL_HD static inline uint32_t sl_group(uint32_t workload, uint32_t table, uint32_t *which) {
  *which = 0;
  if (workload == SL_WL_STORE) return table == 0 ? SL_G_STORE : SL_G_NONE;
  if (workload == SL_WL_SMALLBANK) return table == 0 ? SL_G_SB_SAV : table == 1 ? SL_G_SB_CHK : SL_G_NONE;
  if (workload != SL_WL_TATP || table > 4) return SL_G_NONE;
  *which = table == 4;
  return table == 0 ? SL_G_SUB : table == 1 ? SL_G_SEC : table == 2 ? SL_G_AI : SL_G_SFCF;
}
// draws per subscriber where that is a constant; SL_DRAWS_VAR where the data decides
#define SL_DRAWS_VAR 0xFFFFFFFFu
SL_HD static inline uint32_t sl_draws(uint32_t group) {
  return group == SL_G_STORE ? 12u : group == SL_G_SUB ? 17u : (group == SL_G_AI || group == SL_G_SFCF) ? SL_DRAWS_VAR : 0u;
}
// rows per subscriber of the group's table `which` where that is a constant (else 0)
SL_HD static inline uint32_t sl_rows_fixed(uint32_t group) { return group == SL_G_STORE ? 12u : (group == SL_G_AI || group == SL_G_SFCF) ? 0u : 1u; }

// 3 decimal digits -> 3 BCD nibbles (create_map1000, tatp/udp/tatp.h:18-26); 9 digits of s_id -> sub_nbr (tatp.h:132-144)
SL_HD static inline uint64_t sl_bcd3(uint32_t v) { return ((uint64_t)(v / 100 % 10) << 8) | ((uint64_t)(v / 10 % 10) << 4) | (v % 10); }
SL_HD static inline uint64_t sl_sub_nbr(uint32_t s_id) {
  return sl_bcd3(s_id % 1000) | (sl_bcd3(s_id / 1000 % 1000) << 12) | (sl_bcd3(s_id / 1000000 % 1000) << 24);
}
// select_between_n_and_m_from(seed, {1,2,3,4}, 1, 4) (tatp.h:254-281): a count, then distinct values by rejection; ty = the
// values, 4 bits each, in the order drawn
SL_HD static inline uint32_t sl_pick_types(uint64_t &g, uint32_t *ty) {
  const uint32_t want = sl_lcg_next(g) % 4u + 1u;
  uint32_t used = 0, got = 0, t = 0;
  while (got < want) {
    const uint32_t v = sl_lcg_next(g) % 4u + 1u;
    if (used >> v & 1u) continue;
    used |= 1u << v;
    t |= v << (4u * got++);
  }
  *ty = t;
  return got;
}
// byte `at` of a value whose 8-byte words are w[]
SL_HD static inline void sl_put8(uint64_t *w, uint32_t at, uint32_t byte) { w[at >> 3] |= (uint64_t)(byte & 0xFFu) << (8u * (at & 7u)); }

// The rows of subscriber / account s of `group`, in the reference's insertion order: emit(which, key, w) per row, w = the
// value's 8-byte words (5, or 1 for smallbank), zero where the reference assigns nothing.  g = the stream's state at s's first
// draw, left at the next subscriber's.
template <class E>
SL_HD static inline void sl_gen_sub(uint32_t group, uint64_t s, uint64_t &g, E &&emit) {
  switch (group) {
    case SL_G_STORE:  // store/udp/tatp.h:44-66
      for (uint64_t sf = 1; sf <= 4; sf++)
        for (uint64_t st = 0; st <= 16; st += 8) {
          uint64_t w[5] = {0, 0, 0, 0, 0};
          w[0] = (uint64_t)(sl_lcg_next(g) % 24u + 1u) | 0x5a00ull;  // end_time, numberx[0] = kValMagic
          emit(0u, s | (sf << 32) | (st << 40), w);
        }
      break;
    case SL_G_SB_SAV:
    case SL_G_SB_CHK: {  // smallbank/udp/smallbank.h:105-127: {magic 97 / 98 (:71-73), float 1e9 (:113,121)}
      uint64_t w[5] = {(group == SL_G_SB_SAV ? 97ull : 98ull) | (0x4E6E6B28ull << 32), 0, 0, 0, 0};
      emit(0u, s, w);
      break;
    }
    case SL_G_SUB: {  // tatp/udp/tatp.h:283-309, value = tatp_sub_val_t (tatp.h:160-168)
      uint64_t w[5] = {sl_sub_nbr((uint32_t)s), 0, 0, 0, 0};  // sub_nbr; bytes 8..14 unused
      for (uint32_t i = 0; i < 15; i++) sl_put8(w, 15 + i, sl_lcg_next(g));  // hex[5], bytes[10]
      const uint32_t bits = sl_lcg_next(g) & 0xFFFFu;
      sl_put8(w, 30, bits);
      sl_put8(w, 31, bits >> 8);
      w[4] = 97ull | ((uint64_t)sl_lcg_next(g) << 32);  // msc_location magic, vlr_location
      emit(0u, s, w);
      break;
    }
    case SL_G_SEC: {  // tatp.h:312-327
      uint64_t w[5] = {(uint64_t)(uint32_t)s | (98ull << 32), 0, 0, 0, 0};  // s_id, tatp_sec_sub_magic
      emit(0u, sl_sub_nbr((uint32_t)s), w);
      break;
    }
    case SL_G_AI: {  // tatp.h:330-354
      uint32_t ty;
      const uint32_t k = sl_pick_types(g, &ty);
      for (uint32_t i = 0; i < k; i++) {
        uint64_t w[5] = {99, 0, 0, 0, 0};  // data1 magic
        emit(0u, s | ((uint64_t)(ty >> (4u * i) & 15u) << 32), w);
      }
      break;
    }
    case SL_G_SFCF: {  // tatp.h:357-412
      uint32_t ty;
      const uint32_t k = sl_pick_types(g, &ty);
      for (uint32_t i = 0; i < k; i++) {
        const uint64_t base = s | ((uint64_t)(ty >> (4u * i) & 15u) << 32);
        uint64_t w[5] = {100ull << 24, 0, 0, 0, 0};            // data_b[0] magic
        w[0] |= sl_lcg_next(g) % 100u < 85u ? 1u : 0u;         // is_active
        emit(0u, base, w);
        for (uint64_t st = 0; st <= 16; st += 8) {
          if (sl_lcg_next(g) % 2u == 0) continue;              // present with probability 1/2
          uint64_t c[5] = {101ull << 8, 0, 0, 0, 0};           // numberx[0] magic
          c[0] |= sl_lcg_next(g) % 24u + 1u;                   // end_time
          emit(1u, base | (st << 40), c);
        }
      }
      break;
    }
    default:
      break;
  }
}

// the draw rule alone: the rows subscriber s adds to the group's two tables, the state moved past its draws
struct sl_count_emit {
  uint32_t rows[2] = {0, 0};
  SL_HD inline void operator()(uint32_t which, uint64_t, const uint64_t *) { rows[which]++; }
};
SL_HD static inline void sl_skip_sub(uint32_t group, uint64_t s, uint64_t &g, uint32_t rows[2]) {
  sl_count_emit c;
  sl_gen_sub(group, s, g, c);
  rows[0] = c.rows[0];
  rows[1] = c.rows[1];
}

// ---- host forms of the rule (host functions only below) -----------------------------------------------------------------------
struct sl_place_result {
  uint64_t rows_loaded = 0, foreign_rows = 0, overflow_entries = 0, longest_chain_entries = 0;
  bool too_long = false;  // a bucket beyond KV_MAX_CHAIN entries
};
// The plan of n rows for a table of hash_size global buckets in shard (index, count): order[] = the row numbers in stable
// (local bucket, i) order with the foreign rows last, bucket[i] = row i's local bucket or SR_FOREIGN.  HASH = fasthash64 of a key.
template <class HASH>
static inline sl_place_result sl_plan_host(const uint64_t *keys, uint64_t n, uint64_t hash_size, uint32_t shard_index, uint32_t shard_count,
                                           HASH &&hash, std::vector<uint32_t> &order, std::vector<uint64_t> &bucket) {
  sl_place_result res;
  order.resize(n);
  bucket.resize(n);
  std::iota(order.begin(), order.end(), 0u);
  for (uint64_t i = 0; i < n; i++) bucket[i] = sr_local_bucket(hash(keys[i]) % hash_size, shard_index, shard_count);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return bucket[x] < bucket[y]; });
  uint32_t r = 0;
  for (uint64_t p = 0; p < n; p++) {
    const uint32_t i = order[p];
    if (bucket[i] == SR_FOREIGN) {
      res.foreign_rows++;
      continue;
    }
    r = (p > 0 && bucket[order[p - 1]] == bucket[i]) ? r + 1 : 0;
    res.rows_loaded++;
    if (sr_opens_overflow(r)) res.overflow_entries++;
    res.longest_chain_entries = std::max<uint64_t>(res.longest_chain_entries, sr_entries(r + 1u));
    if (sl_chain_too_long(sr_entries(r + 1u))) res.too_long = true;
  }
  return res;
}
// ... and the plan carried out on a table that holds nothing (the caller has compared res.overflow_entries with t.pool_cap)
static inline void sl_build_host(const kv_tab &t, const uint64_t *keys, const uint32_t *vers, const uint8_t *vals, uint64_t n,
                                 const std::vector<uint32_t> &order, const std::vector<uint64_t> &bucket) {
  uint32_t pool = 0, r = 0, link = KV_NULL, prev_pool = 0;
  for (uint64_t p = 0; p < n; p++) {
    const uint32_t i = order[p];
    const uint64_t b = bucket[i];
    if (b == SR_FOREIGN) break;  // (foreign rows sort last)
    r = (p > 0 && bucket[order[p - 1]] == b) ? r + 1 : 0;
    if (sr_opens_entry(r)) {
      const uint32_t x = sr_chain_pos(r);
      const uint32_t mine = pool;
      link = sr_link(x, mine);
      if (x >= 1) pool++;
      kv_hdr *h = kv_entry_hdr(t, b, link);
      h->validw = 0;
      h->next = sl_next(x, prev_pool);
      kv_entry_hdr(t, b, KV_INLINE)->head = link;  // (the newest entry so far)
      prev_pool = mine;
    }
    uint8_t *e = kv_entry_ptr(t, b, link);
    kv_hdr *h = (kv_hdr *)e;
    const uint32_t s = sr_slot(r);
    h->key[s] = keys[i];
    h->ver[s] = vers ? vers[i] : 0u;
    e[KV_VALID_OFF + s] = 1;
    memcpy(e + KV_VAL_OFF + s * t.val_size, vals + (uint64_t)i * t.val_size, t.val_size);
  }
  *t.pool_top = pool;
}

// the tile table of a data-dependent group, continued from where it stands to cover `n_subs` subscribers: state[k] = the stream's
// state at subscriber k * SL_TILE, rows[which][k] = the rows of subscribers 0 .. k * SL_TILE - 1.  Entry k exists once
// subscriber k * SL_TILE - 1 has been walked, so the table is a prefix of the group's, whatever n asked for it.
struct sl_tiles {
  std::vector<uint64_t> state, rows[2];
  uint64_t g = SL_SEED, done[2] = {0, 0};  // the state and rows behind the last whole tile walked
};
static inline void sl_tile_walk(uint32_t group, sl_tiles &tl, uint64_t n_subs) {
  const uint64_t want = n_subs / SL_TILE + 1;  // entries 0 .. n_subs / SL_TILE
  while (tl.state.size() < want) {
    const uint64_t k = tl.state.size();
    if (k > 0)
      for (uint64_t s = (k - 1) * SL_TILE; s < k * SL_TILE; s++) {
        uint32_t r[2];
        sl_skip_sub(group, s, tl.g, r);
        tl.done[0] += r[0];
        tl.done[1] += r[1];
      }
    tl.state.push_back(tl.g);
    tl.rows[0].push_back(tl.done[0]);
    tl.rows[1].push_back(tl.done[1]);
  }
}
