// traffic_report.h -- what one batch of wire messages looks like to the passes: one source for the kernels (k_traffic.hip:
// struct dint_traffic_report, include/dint_abi.h) and the host form over caller-provided memory (dint_traffic_report_host,
// include/dint_driver.h), as state_stats.h is for the table report.  Integer arithmetic only; nothing is written.
//
//   decode    table t, key k and type byte y of a wire message (include/dint_abi.h structs, dint_amd/wire.py):
//               lock_fasst {u8 type; u32 lid; u32 ver}            t = 0, k = lid, y = type
//               lock_2pl   {u8 action; u32 lid; u8 type}          t = 0, k = lid, y = action; the lock-type byte decides the class
//               store      {u8 type; u64 key; ...}                t = 0
//               tatp / smallbank {u8 ord, type, table; u64 key; ...}
//             A reply is decoded at the same offsets; only its type byte is used.
//   class     of a REQUEST, from y:
//               READ    fasst 0; store 0; tatp 0; smallbank 17 (WARMUP_READ)
//               LOCK    an acquire: fasst 1; 2pl action 0; tatp 1; smallbank 0, 1
//               UNLOCK  fasst 2 (ABORT); 2pl action 1; tatp 2 (ABORT); smallbank 2, 3
//               WRITE   row- or version-changing: fasst 3; store 1, 2; tatp 12, 13, 18, 19, 22, 23; smallbank 4, 5
//               LOG     tatp 14, 24; smallbank 6
//               OTHER   anything else -- reply codes sent as requests, unknown bytes, and a lock_2pl message whose lock-type byte is
//                       neither SHARED (0) nor EXCLUSIVE (1), which the server counts as a bad request
//             SLOT: the request works on the key's lock slot (tatp / smallbank): LOCK, UNLOCK, or a WRITE at the primary --
//             tatp 12, 18, 22, smallbank 4 -- which releases the lock it commits under
//   flags     of a REPLY, from its type byte:
//               REJECT  fasst 6; 2pl 3, 4; store 4, 6, 9; tatp 5, 8, 11, 28; smallbank 8, 10, 16
//               MISS    store 7; tatp 6
//   keyed     t < n_tables and class != LOG.  A request with t >= n_tables counts in bad_table and nowhere else; a LOG request counts
//             in the two type histograms and log_requests only.  Classes, flags, keys, units and slots are over the keyed requests.
//   unit      what requests must be applied in order on: lock tables fasthash64(&lid, 4) % n_slots; kv
//             (t, fasthash64(&key, 8) % hash_size[t]) -- GLOBAL sizes, whatever the engine's shard
//   lock slot tatp / smallbank: (t, fasthash64(&key, 8) % (4 hash_size[t]))
// A group id (unit or lock slot) is one 64-bit word, table << TR_GROUP_TABLE_SHIFT | id: ascending words = ascending (table, id).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/dint_abi.h"
#include "dint_device.h"

#if defined(__HIPCC__)
#define TR_HD __host__ __device__
#else
#define TR_HD
#endif

#define TR_MAX_TABLES 5u
#define TR_TYPE_BINS 32u
#define TR_HIST_BINS 25u
#define TR_GROUP_TABLE_SHIFT 60u
#define TR_NO_GROUP (~0ull)  // (table 15: no workload has it)

enum : uint32_t { TR_READ = 0, TR_LOCK, TR_UNLOCK, TR_WRITE, TR_LOG, TR_OTHER, TR_CLASSES };
// the meta word of a request: class in bits 0..2, table in 3..5 (7: not keyed), then the flags
enum : uint32_t { TR_M_CLASS = 7u, TR_M_TABLE_SHIFT = 3u, TR_M_REJECT = 1u << 6, TR_M_MISS = 1u << 7, TR_M_SLOT = 1u << 8, TR_NOT_KEYED = 7u };

// the words of a result block (device: unsigned long long[TR_WORDS]); the first TR_W_KEY_HIST are dint_traffic_report's scalars in
// the struct's order
enum : uint32_t {
  TR_W_N = 0, TR_W_KEYED, TR_W_BAD_TABLE, TR_W_LOG, TR_W_READS, TR_W_LOCKS, TR_W_UNLOCKS, TR_W_WRITES, TR_W_OTHERS, TR_W_REJECTS, TR_W_MISSES,
  TR_W_DKEYS, TR_W_DUNITS, TR_W_DSLOTS, TR_W_MAX_KEY, TR_W_MAX_UNIT_REQ, TR_W_MAX_UNIT, TR_W_MAX_UNIT_TABLE, TR_W_SH_UNITS, TR_W_SH_UNIT_REQ,
  TR_W_SH_UNIT_REJ, TR_W_SH_SLOTS, TR_W_SH_SLOT_REQ, TR_W_SH_SLOT_REJ, TR_W_N_BY_REQ, TR_W_N_BY_REJ, TR_W_TEMP, TR_W_RESERVED,
  TR_W_KEY_HIST = 32, TR_W_UNIT_HIST = TR_W_KEY_HIST + TR_HIST_BINS, TR_W_REQ_TYPES = TR_W_UNIT_HIST + TR_HIST_BINS,
  TR_W_REP_TYPES = TR_W_REQ_TYPES + TR_MAX_TABLES * TR_TYPE_BINS, TR_WORDS = TR_W_REP_TYPES + TR_MAX_TABLES * TR_TYPE_BINS
};
static_assert(sizeof(struct dint_traffic_report) == 8 * TR_WORDS && offsetof(struct dint_traffic_report, key_hist) == 8 * TR_W_KEY_HIST &&
                  offsetof(struct dint_traffic_report, unit_hist) == 8 * TR_W_UNIT_HIST && offsetof(struct dint_traffic_report, req_types) == 8 * TR_W_REQ_TYPES &&
                  offsetof(struct dint_traffic_report, rep_types) == 8 * TR_W_REP_TYPES && offsetof(struct dint_traffic_report, temp_bytes) == 8 * TR_W_TEMP &&
                  offsetof(struct dint_traffic_report, misses) == 8 * TR_W_MISSES && offsetof(struct dint_traffic_report, shared_slot_rejects) == 8 * TR_W_SH_SLOT_REJ,
              "the words of traffic_report.h are the fields of dint_traffic_report");
static_assert(sizeof(dint_traffic_key) == 48, "a list entry is 48 bytes");

// where the fields of a message are (byte offsets; table == TR_NO_FIELD: the workload has one table)
#define TR_NO_FIELD 0xFFFFFFFFu
struct tr_format {
  uint32_t msg, type, table, key, key_bytes, ltype;  // ltype: lock_2pl's lock-type byte
};
TR_HD static inline tr_format tr_format_of(uint32_t workload) {
  switch (workload) {
    case DINT_WL_FASST: return {9, 0, TR_NO_FIELD, 1, 4, TR_NO_FIELD};
    case DINT_WL_2PL: return {6, 0, TR_NO_FIELD, 1, 4, 5};
    case DINT_WL_STORE: return {53, 0, TR_NO_FIELD, 1, 8, TR_NO_FIELD};
    case DINT_WL_TATP: return {55, 1, 2, 3, 8, TR_NO_FIELD};
    case DINT_WL_SMALLBANK: return {23, 1, 2, 3, 8, TR_NO_FIELD};
    default: return {0, 0, TR_NO_FIELD, 0, 0, TR_NO_FIELD};
  }
}
TR_HD static inline bool tr_workload_ok(uint32_t workload) { return tr_format_of(workload).msg != 0; }
TR_HD static inline bool tr_has_slots(uint32_t workload) { return workload == DINT_WL_TATP || workload == DINT_WL_SMALLBANK; }

// the geometry a report is taken under: global sizes only
struct tr_geom {
  uint32_t workload, n_tables;
  dint_mod unit[TR_MAX_TABLES];  // % n_slots / % hash_size[t]
  dint_mod slot[TR_MAX_TABLES];  // % (4 hash_size[t])  (tatp / smallbank)
};

// the key of a message, byte by byte (a message sits at any address)
template <class P>
TR_HD static inline uint64_t tr_load_key(P m, const tr_format &f) {
  uint64_t k = 0;
  for (uint32_t b = 0; b < f.key_bytes; b++) k |= (uint64_t)m[f.key + b] << (8 * b);
  return k;
}
TR_HD static inline uint32_t tr_type_bin(uint32_t y) { return y < TR_TYPE_BINS - 1 ? y : TR_TYPE_BINS - 1; }

// class of a request (ltype: lock_2pl's lock-type byte, else ignored), with TR_M_SLOT where it applies
TR_HD static inline uint32_t tr_class(uint32_t workload, uint32_t y, uint32_t ltype) {
  switch (workload) {
    case DINT_WL_FASST:
      return y == 0 ? TR_READ : y == 1 ? TR_LOCK : y == 2 ? TR_UNLOCK : y == 3 ? TR_WRITE : TR_OTHER;
    case DINT_WL_2PL:
      if (ltype > 1) return TR_OTHER;
      return y == 0 ? TR_LOCK : y == 1 ? TR_UNLOCK : TR_OTHER;
    case DINT_WL_STORE:
      return y == 0 ? TR_READ : (y == 1 || y == 2) ? TR_WRITE : TR_OTHER;
    case DINT_WL_TATP:
      if (y == 0) return TR_READ;
      if (y == 1) return TR_LOCK | TR_M_SLOT;
      if (y == 2) return TR_UNLOCK | TR_M_SLOT;
      if (y == 12 || y == 18 || y == 22) return TR_WRITE | TR_M_SLOT;
      if (y == 13 || y == 19 || y == 23) return TR_WRITE;
      if (y == 14 || y == 24) return TR_LOG;
      return TR_OTHER;
    case DINT_WL_SMALLBANK:
      if (y == 0 || y == 1) return TR_LOCK | TR_M_SLOT;
      if (y == 2 || y == 3) return TR_UNLOCK | TR_M_SLOT;
      if (y == 4) return TR_WRITE | TR_M_SLOT;
      if (y == 5) return TR_WRITE;
      if (y == 6) return TR_LOG;
      if (y == 17) return TR_READ;
      return TR_OTHER;
    default: return TR_OTHER;
  }
}
// flags of a reply (TR_M_REJECT / TR_M_MISS)
TR_HD static inline uint32_t tr_reply_flags(uint32_t workload, uint32_t y) {
  switch (workload) {
    case DINT_WL_FASST: return y == 6 ? TR_M_REJECT : 0;
    case DINT_WL_2PL: return (y == 3 || y == 4) ? TR_M_REJECT : 0;
    case DINT_WL_STORE: return (y == 4 || y == 6 || y == 9) ? TR_M_REJECT : y == 7 ? TR_M_MISS : 0;
    case DINT_WL_TATP: return (y == 5 || y == 8 || y == 11 || y == 28) ? TR_M_REJECT : y == 6 ? TR_M_MISS : 0;
    case DINT_WL_SMALLBANK: return (y == 8 || y == 10 || y == 16) ? TR_M_REJECT : 0;
    default: return 0;
  }
}

// one request (and its reply, rep == nullptr: none) decoded: *key, the type bytes, and the meta word -- table TR_NOT_KEYED for a
// request that is not keyed; *t_out = the table byte as sent (histograms take t < n_tables, LOG requests included)
template <class P>
TR_HD static inline uint32_t tr_decode(const tr_geom &g, const tr_format &f, P req, P rep, bool has_rep, uint64_t *key, uint32_t *t_out,
                                       uint32_t *y_req, uint32_t *y_rep) {
  const uint32_t t = f.table == TR_NO_FIELD ? 0u : (uint32_t)req[f.table];
  const uint32_t y = req[f.type];
  *t_out = t;
  *y_req = y;
  *y_rep = has_rep ? (uint32_t)rep[f.type] : 0u;
  *key = tr_load_key(req, f);
  if (t >= g.n_tables) return TR_NOT_KEYED << TR_M_TABLE_SHIFT | TR_OTHER;
  const uint32_t c = tr_class(g.workload, y, f.ltype == TR_NO_FIELD ? 0u : (uint32_t)req[f.ltype]);
  if ((c & TR_M_CLASS) == TR_LOG) return TR_NOT_KEYED << TR_M_TABLE_SHIFT | TR_LOG;
  return c | t << TR_M_TABLE_SHIFT | (has_rep ? tr_reply_flags(g.workload, *y_rep) : 0u);
}

// the unit / the lock slot of a keyed request's (table, key), as a group word
TR_HD static inline uint64_t tr_unit(const tr_geom &g, uint32_t t, uint64_t key) {
  const bool lock = g.workload == DINT_WL_FASST || g.workload == DINT_WL_2PL;
  const uint64_t h = lock ? dint_hash_lid((uint32_t)key) : dint_hash_key(key);
  return (uint64_t)t << TR_GROUP_TABLE_SHIFT | dint_fastmod(h, g.unit[t]);
}
TR_HD static inline uint64_t tr_slot(const tr_geom &g, uint32_t t, uint64_t key) {
  return (uint64_t)t << TR_GROUP_TABLE_SHIFT | dint_fastmod(dint_hash_key(key), g.slot[t]);
}
// bin of a per-key / per-unit request count (c >= 1; c <= 2^24 by the call's contract, so the last bin is 2^24 alone)
TR_HD static inline uint32_t tr_count_bin(uint32_t c) {
  uint32_t b = 0;
  while (b + 1 < TR_HIST_BINS && (c >> (b + 1))) b++;
  return b;
}
