// state_sync.h -- comparing the rows of two engines and making one equal to the other: one source for the kernels
// (k_state.hip: dint_state_digest / dint_state_diff / dint_state_repair, include/dint_abi.h) and the host forms
// (dint_state_row_hash_host / dint_state_digest_host / dint_state_diff_host, include/dint_driver.h), as log_replay.h is for
// the log replay.
//
// "State" is rows only: per table the multiset of valid (key, ver, val) slots.  Lock words, the log ring, the pool's free
// lists and the chain layout are per server and transient; a replica rebuilt from a log has other chains than its primary.
//
//   row hash  fasthash64(canonical bytes, len, 0xdeadbeef) (lock_fasst/udp/utils.h:16-53) over
//             key (8, LE) | ver (4, LE) | table (1) | 0 0 0 | val (val_size): 56 bytes (store / tatp) or 24 (smallbank) --
//             whole 8-byte blocks, so the tail switch of fasthash64 is never entered
//   digest    {rows, sum of the row hashes mod 2^64, xor of the row hashes}: commutative, so it depends on neither the
//             chain layout nor the bucket order; duplicate rows count once each
//   diff      per bucket, over the VISIBLE rows (per key the first valid slot in chain order -- what a READ returns):
//             first a's rows that b lacks or holds differently, in a's chain order, then the rows only b has, in b's
// Integer arithmetic only, so host and device produce the same bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "log_replay.h"

#if defined(__HIPCC__)
#define SS_HD __host__ __device__
#else
#define SS_HD
#endif

#define SS_SEED 0xdeadbeefULL
#define SS_M 0x880355f21e6d1965ULL

SS_HD static inline uint64_t ss_mix(uint64_t h) {  // (dint_device.h dint_mix; restated so that a plain C++ compiler takes this header)
  h ^= h >> 23;
  h *= 0x2127599bf4325c37ULL;
  h ^= h >> 47;
  return h;
}
// fasthash64 over whole 8-byte blocks: start with the length in bytes, feed the blocks in order, finish
SS_HD static inline uint64_t ss_hash_begin(uint32_t len) { return SS_SEED ^ ((uint64_t)len * SS_M); }
SS_HD static inline uint64_t ss_hash_block(uint64_t h, uint64_t v) { return (h ^ ss_mix(v)) * SS_M; }
SS_HD static inline uint64_t ss_hash_end(uint64_t h) { return ss_mix(h); }
// the second block of a row's canonical bytes
SS_HD static inline uint64_t ss_row_word1(uint32_t ver, uint32_t table) { return (uint64_t)ver | ((uint64_t)(table & 0xFFu) << 32); }
// the row hash; val_word(k) = the k-th little-endian 8-byte word of the value (val_size = 40 or 8)
template <class ValWord>
SS_HD static inline uint64_t ss_row_hash(uint64_t key, uint32_t ver, uint32_t table, uint32_t val_size, ValWord val_word) {
  uint64_t h = ss_hash_begin(16u + val_size);
  h = ss_hash_block(h, key);
  h = ss_hash_block(h, ss_row_word1(ver, table));
  for (uint32_t k = 0; k < val_size / 8; k++) h = ss_hash_block(h, val_word(k));
  return ss_hash_end(h);
}

struct ss_digest {
  uint64_t rows, sum, xr;
};
SS_HD static inline void ss_digest_add(ss_digest &d, uint64_t row_hash) { d.rows++; d.sum += row_hash; d.xr ^= row_hash; }
SS_HD static inline void ss_digest_merge(ss_digest &d, const ss_digest &o) { d.rows += o.rows; d.sum += o.sum; d.xr ^= o.xr; }

// ---- the diff rule of one bucket --------------------------------------------------------------------------------
// What has to be done to b: SS_ONLY_A = insert a's row, SS_VAL / SS_VER = overwrite b's row with a's (value differs, whatever
// the version / the version alone differs), SS_ONLY_B = delete b's row.  The order of the enum is the order of dint_diff_stats.
enum : uint32_t { SS_ONLY_A = 0, SS_ONLY_B = 1, SS_VAL = 2, SS_VER = 3 };

// A row list L (a bucket's rows in chain order) is anything with
//   pos  begin()          first valid row, or an end position
//   pos  next(pos)        the valid row after it, or an end position
//   bool ok(pos)          not an end position
//   u64  key(pos), u32 ver(pos), u32 val32(pos, w)   (w-th little-endian 4-byte word of the value)
//   pos  find(key)        the first valid row with this key (the VISIBLE one), or an end position
//   bool same(pos, pos)
// `bound` limits every loop (a corrupt chain must never hang a GPU); emit(kind, list, pos) is called once per record, in the
// contract's order.
template <class LA, class LB, class Emit>
SS_HD static inline void ss_bucket_diff(const LA &a, const LB &b, uint32_t val_size, uint32_t bound, Emit &emit) {
  uint32_t steps = 0;
  for (auto p = a.begin(); a.ok(p) && steps < bound; p = a.next(p), steps++) {
    const uint64_t k = a.key(p);
    if (!a.same(a.find(k), p)) continue;  // shadowed by an earlier row with the same key
    const auto q = b.find(k);
    if (!b.ok(q)) {
      emit(SS_ONLY_A, a, p);
      continue;
    }
    bool val_eq = true;
    for (uint32_t w = 0; w < val_size / 4; w++) val_eq = val_eq && a.val32(p, w) == b.val32(q, w);
    if (!val_eq) emit(SS_VAL, a, p);
    else if (a.ver(p) != b.ver(q)) emit(SS_VER, a, p);
  }
  steps = 0;
  for (auto q = b.begin(); b.ok(q) && steps < bound; q = b.next(q), steps++) {
    const uint64_t k = b.key(q);
    if (!b.same(b.find(k), q)) continue;
    if (!a.ok(a.find(k))) emit(SS_ONLY_B, b, q);
  }
}

// the record of one difference, as the 16 little-endian words of an LrRecord: a's row as it is, or a delete of b's row
// (val and ver zero)
template <class L, class P>
SS_HD static inline void ss_fill_record(uint32_t w[16], uint32_t kind, const L &l, P p, uint32_t table, uint32_t val_size) {
  for (uint32_t k = 0; k < 16; k++) w[k] = 0;
  const uint64_t key = l.key(p);
  w[0] = (uint32_t)key;
  w[1] = (uint32_t)(key >> 32);
  if (kind == SS_ONLY_B) {
    w[13] = 1u | ((table & 0xFFu) << 8);  // is_del, table
    return;
  }
  for (uint32_t k = 0; k < val_size / 4; k++) w[2 + k] = l.val32(p, k);
  w[12] = l.ver(p);
  w[13] = (table & 0xFFu) << 8;
}
static_assert(sizeof(LrRecord) == 64 && offsetof(LrRecord, ver) == 48 && offsetof(LrRecord, is_del) == 52 && offsetof(LrRecord, table) == 53,
              "the diff writes canonical log records");
