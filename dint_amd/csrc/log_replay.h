// log_replay.h -- what a drained log record becomes when it is replayed into a replica, one source for the host form
// (dint_log_classify_host, k_replay.hip) and the replay kernels (k_replay.hip), as lock_clients.h is for the lock clients.
//
// The client sends, right after the log record, the backup operation on the same row (tatp/caladan/client_udp_shard.cc:
// 486-570): COMMIT_BCK for a row that exists, INSERT_BCK for one that does not yet, DELETE_BCK after a DELETE_LOG.  A log
// record does not say which of the first two it was; the replay learns it from the row's state at that point of the log:
// what the previous record on the same row left behind, or -- for the first record of a row -- what the replica holds.
// dint_amd/recovery.py apply_log states the same rule in numpy.  smallbank has neither inserts nor deletes: COMMIT_BCK.
// Integer arithmetic only, so host and device choose the same bytes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LR_HD __host__ __device__
#else
#define LR_HD
#endif

#pragma pack(push, 1)
struct LrRecord {  // the canonical 64-byte record of every log ring (include/dint_abi.h dint_read_log)
  uint64_t key;
  uint8_t val[40];
  uint32_t ver;
  uint8_t is_del;
  uint8_t table;
  uint8_t pad[10];
};
struct LrTatpMsg {  // tatp/udp/net.h:54-66
  uint8_t ord, type, table;
  uint64_t key;
  uint8_t val[40];
  uint32_t ver;
};
struct LrSbMsg {  // smallbank/udp/net.h:40-50
  uint8_t ord, type, table;
  uint64_t key;
  uint8_t val[8];
  uint32_t ver;
};
#pragma pack(pop)
static_assert(sizeof(LrRecord) == 64 && sizeof(LrTatpMsg) == 55 && sizeof(LrSbMsg) == 23, "packed wire structs");

enum : uint8_t {  // tatp/udp/net.h:15-52, smallbank/udp/net.h:15-38
  LR_T_READ = 0, LR_T_GRANT_READ = 4, LR_T_COMMIT_BCK = 13, LR_T_COMMIT_BCK_ACK = 16, LR_T_INSERT_BCK = 19,
  LR_T_INSERT_BCK_ACK = 21, LR_T_DELETE_BCK = 23, LR_T_DELETE_BCK_ACK = 26,
  LR_S_COMMIT_BCK = 5, LR_S_COMMIT_BCK_ACK = 14
};

// rows are grouped by this word: the table above the key (tatp keys use < 48 bits)
LR_HD static inline uint64_t lr_row(uint8_t table, uint64_t key) { return ((uint64_t)table << 60) ^ key; }

// the tatp backup operation of a record; `exists` = the row exists just before the record
LR_HD static inline uint8_t lr_tatp_type(bool is_del, bool exists) {
  return is_del ? LR_T_DELETE_BCK : exists ? LR_T_COMMIT_BCK : LR_T_INSERT_BCK;
}
// does the row exist before a record that is NOT the first of its row: the previous record on the row left it there
// unless it was a delete
LR_HD static inline bool lr_exists_after(uint8_t prev_is_del) { return prev_is_del == 0; }
