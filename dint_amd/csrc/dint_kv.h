// dint_kv.h -- HBM key-value tables of the store / tatp / smallbank workloads (k_kv.hip).
#pragma once
#include <cstdlib>
#include <utility>
#include <vector>

#include "dint_kernels.h"
#include "dint_kv_core.h"
#include "state_block.h"
#include "state_image.h"
#include "state_locks.h"
#include "state_route.h"

#define DINT_KV_MAX_TABLES 5
#define DINT_KV_CTL_BYTES (64 + 24 * KV_NLISTS)  // per table: pool_top, free_head[], pend_head[2][] (two sets: dint_kv_core.h, kv_pool_rotate)
#define DINT_KV_TRACE_WORDS ((size_t)DINT_KV_PMAX * 16 + 16 * 8192)  // per bin 16 words, then per workgroup 16
#define DINT_KV_LOAD_OP 0xF0u  // internal request type: insert a row with the version carried in msg.ver

// everything the kernels need about the tables; lives in device memory (d_dev) and in a host mirror
struct kv_dev {
  kv_tab tab[DINT_KV_MAX_TABLES];
  dint_mod mod[DINT_KV_MAX_TABLES];      // % hash_size (global bucket)
  dint_mod lockmod[DINT_KV_MAX_TABLES];  // % (4 * hash_size)  (tatp/udp/tatp.h:12-14)
  uint32_t gk_base[DINT_KV_MAX_TABLES];  // group key of local bucket 0 of each table
  uint32_t n_tables;
  uint32_t shard_index, shard_count;
  uint32_t same_key;  // tatp, DINT_FLAG_LOCK_SAME_KEY: lock slots remember their owner's key (tatp/ebpf/lock_kern.c)
  uint32_t pass_ins[DINT_KV_MAX_TABLES];  // LDS copies only (k_kv_dev.h, kv_dev_word): INSERT requests of the pass per table; 2^32 - 1 in memory
};

// Tuning / test knobs of the kv passes, read from the environment ONCE, when the engine is created (r01-r05 read them with
// getenv at every launch -- ten per pass; VERDICT / ADVICE r05).  Tests set the variable before they create their engine.
struct dint_kv_knobs {
  uint32_t coarse_load = 512;   // DINT_KV_COARSE_LOAD: records per coarse bin
  uint32_t cap = 0;             // DINT_KV_CAP: records a coarse bin holds in place (0 = cap_mult x the mean load + 64)
  uint32_t lcap = 1024;         // DINT_KV_LCAP: records of a bin's small subs resolved from LDS
  uint32_t cap_mult = 64;       // DINT_KV_CAP_MULT
  uint32_t rpt = 0;             // DINT_KV_RPT: requests per thread of k_kv_part (0 = by pass size)
  uint32_t no_bm = 0;           // DINT_KV_NO_BM: kv_big_bin sorts where it would rank by index bitmap
  uint32_t hot_min = 0;         // DINT_KV_HOT_MIN
  uint32_t no_split = 0;        // DINT_KV_NO_SPLIT: r04's kv_big_bin for every big sub
  uint32_t split_min = 65;      // DINT_KV_SPLIT_MIN
  uint32_t split_target = 384;  // DINT_KV_SPLIT_TARGET
  uint32_t one_big_kernel = 0;  // DINT_KV_ONE_BIG_KERNEL: no k_kv_hot launch
  uint32_t workers = 96;        // DINT_KV_WORKERS: hot-key workers per engine of k_kv_pass
  uint32_t part_first = 0;      // DINT_KV_PART_FIRST: k_kv_pass places the next partition's tiles before (1) / behind (0) the workers
  uint32_t sb_split_min = 65;   // DINT_KV_SB_SPLIT_MIN: smallbank, the smallest big sub whose row is answered in pieces (65: every big sub; 0: never -- r05's kv_big_bin)
  uint32_t sb_npmax = 128;      // DINT_KV_SB_NPMAX: smallbank, pieces of one row at most (<= KSB_NPMAX; x 384 requests: 49,000 -- a bigger row goes the old way)
  uint32_t sb_workers = 130;    // DINT_KV_SB_WORKERS: smallbank, workers per engine of k_kv_pass (>= KSB_NPMAX + 2: a row's pieces wait for each other; 0: every item in k_kv_big)
  uint32_t sb_late_grid = 32;   // DINT_KV_SB_LATE_GRID: smallbank, workgroups per engine of the k_kv_big launch behind the workers
  uint32_t residency = 0;       // workgroups of the pieces' kernel the device holds at once (kv_piece_residency)
  uint32_t no_fuse = 0;         // DINT_KV_NO_FUSE: k_kv_resolve and k_kv_hot / k_kv_hot_part as launches of their own, not k_kv_pass
  uint32_t no_ahead = 0;        // DINT_KV_NO_AHEAD: never run a pass's partition beside the previous pass's hot keys
  uint32_t late_grid = 8;       // DINT_KV_LATE_GRID: workgroups of the k_kv_big launch behind k_kv_hot (DINT_KV_LATE_BIG)
  uint32_t exp_no_late = 0;     // DINT_EXP_NO_LATE: experiments only -- no launch behind k_kv_hot at all (late items stay unanswered)
  uint32_t late_fat = 0;        // DINT_KV_LATE_FAT: k_kv_late at 256 VGPRs (no spills, but its workgroups want an empty compute unit)
  uint32_t late_big = 0;        // DINT_KV_LATE_BIG: what k_kv_hot leaves goes to k_kv_big (r05) instead of k_kv_late
};

struct dint_kv {
  uint32_t workload = 0;
  uint32_t n_tables = 0;
  uint32_t val_size = 0;
  int force_rounds = 0;  // DINT_FLAG_KV_ROUNDS: never use the closed-form same-key path (A/B and parity testing)
  uint64_t hash_size[DINT_KV_MAX_TABLES] = {0, 0, 0, 0, 0};  // global bucket counts
  kv_dev h{};                // host mirror (device pointers inside)
  kv_dev *d_dev = nullptr;   // device copy
  uint8_t *d_ctl = nullptr;  // pool_top / free_head / pend_head words of all tables
  uint64_t *d_trace = nullptr;  // DINT_KV_TRACE=1: [DINT_PMAX][16] per-wave s_memtime stamps of the last resolve launch
  size_t entry_bytes[DINT_KV_MAX_TABLES] = {0, 0, 0, 0, 0};
  dint_kv_knobs knobs;
};

// records a coarse bin of a kv pass holds IN PLACE, in units of the mean load of a bin (engine.hip sizes the scratch for it,
// k_kv.hip's kv_fill_pass sets the pass's `cap`); DINT_KV_CAP_MULT overrides (2 = r04 / r05: a hot key's bin overflows)
static inline uint32_t dint_kv_cap_mult() {
  const char *v = getenv("DINT_KV_CAP_MULT");
  const unsigned long m = v && *v ? strtoul(v, nullptr, 10) : 64ul;
  return (uint32_t)(m < 2 ? 2 : m > 256 ? 256 : m);
}
// the global bucket counts of a kv workload's tables for dint_config.n_rows (0 = the reference's size), as dint_kv_create builds
// them and dint_records_route_host routes by them; returns the number of tables (store / tatp / smallbank: 1 / 5 / 2)
static inline uint32_t dint_kv_hash_sizes(uint32_t workload, uint64_t n_rows, uint64_t hs[DINT_KV_MAX_TABLES], uint32_t *val_size) {
  uint32_t n_tables;
  for (uint32_t t = 0; t < DINT_KV_MAX_TABLES; t++) hs[t] = 0;
  if (workload == DINT_WL_STORE) {
    const uint64_t n = n_rows ? n_rows : 2000000ull;  // store/udp/tatp.h:10
    n_tables = 1;
    *val_size = 40;
    hs[0] = n * 18 / 4;  // store/udp/server.cc:112-114: 12 rows per subscriber * 3/2 / 4 slots
  } else if (workload == DINT_WL_TATP) {
    const uint64_t n = n_rows ? n_rows : 7000000ull;  // tatp/udp/tatp.h:28
    n_tables = 5;
    *val_size = 40;
    hs[0] = hs[1] = n * 3 / 2 / 4;   // tatp/udp/server_shard.cc:75-76
    hs[2] = hs[3] = n * 15 / 4 / 4;  // :77-78
    hs[4] = n * 45 / 8 / 4;          // :79
  } else {
    const uint64_t n = n_rows ? n_rows : 24000000ull;  // smallbank/udp/smallbank.h:17
    n_tables = 2;
    *val_size = 8;
    hs[0] = hs[1] = n * 3 / 2 / 4;  // smallbank/udp/server_shard.cc:75-76
  }
  for (uint32_t t = 0; t < n_tables; t++)
    if (hs[t] == 0) hs[t] = 1;
  return n_tables;
}
int dint_kv_create(dint_kv *kv, uint32_t workload, uint64_t n_rows, dint_shard shard, uint32_t pool_entries = 0,
                   uint32_t flags = 0);
void dint_kv_destroy(dint_kv *kv);
std::vector<std::pair<void *, size_t>> dint_kv_regions(dint_kv *kv);
// valid rows of `table` in bucket order, chain order inside a bucket; returns the row count
int64_t dint_kv_dump_rows(dint_kv *kv, uint32_t table, uint64_t *keys, uint32_t *vers, uint8_t *vals, uint64_t cap);
// lock words, index = q * n_local + local bucket  (== lock_hash when unsharded)
int64_t dint_kv_read_locks(dint_kv *kv, uint32_t table, uint32_t *a, uint32_t *b, uint64_t cap);
// one pass (n <= DINT_MICRO and, when a log is attached, n <= log.cap).  load_mode: accept DINT_KV_LOAD_OP
// rows and ignore rows of other shards silently.
// `view`: where request i lives (contiguous array, or the segments of a multi-GPU exchange buffer)
// Look-ahead (r06; store / tatp): `next` = the batch of the engine's NEXT pass, complete in device memory in the order of
// `st`: its partition stage (k_kv_part: no table access) then runs in ONE launch with this pass's hot keys (k_kv_hot_part),
// and that next pass is launched with part_done = true.  dint_kv_ahead_ok says whether a pass of this engine can take one.
struct dint_kv_ahead {
  const void *d_req;
  void *d_rep;
  uint32_t n;
  dint_view view;
};
bool dint_kv_ahead_ok(const dint_kv &kv, int load_mode);
bool dint_kv_one_launch(const dint_kv &kv, int load_mode);
void dint_launch_kv(const void *d_req, void *d_rep, uint32_t n, const dint_kv &kv, dint_log log, dint_scratch s,
                    int load_mode, hipStream_t st, hipEvent_t *ev, const dint_view &view = dint_flat_view(),
                    bool part_done = false, const dint_kv_ahead *next = nullptr);
// the passes of several engines of one kv workload in one launch set (grid.y = engine), all on one stream: what a
// closed-loop epoch or an exchange step hands the GPU's shard servers at the same moment (n > 0 for every engine)
#define DINT_KV_MULTI_MAX 4u
struct dint_kv_pass {
  const void *d_req;
  void *d_rep;
  uint32_t n;
  const dint_kv *kv;
  dint_log log;
  dint_scratch s;
  dint_view view;
};
void dint_launch_kv_multi(const dint_kv_pass *p, uint32_t n_eng, hipStream_t st, bool part_done = false, const dint_kv_pass *next = nullptr);
bool dint_kv_multi_ahead_ok(const dint_kv &kv);
void dint_launch_home_kv(const void *d_req, uint32_t n, const dint_kv &kv, uint8_t *d_home, hipStream_t st);
// wire message size / field offsets of a kv workload
struct dint_kv_fmt {
  uint32_t msg, type, table, key, val, ver, val_size;  // table == 0xFFFFFFFF: no table field
};
dint_kv_fmt dint_kv_format(uint32_t workload);

// ---- state sync (k_state.hip; state_sync.h): digest / diff / repair of the tables' rows ---------------------------
struct dint_state_scratch {
  unsigned long long *words;  // [32] device words: [0..3] the diff's records by kind (state_sync.h SS_*), [4] their number,
                              // [8] the repair's "records out of order" flag, [9..12] {updated, inserted, deleted, refused}, [14] the home check's flag,
                              // [16 ..] the digest: {rows, sum, xor, 0} per table
  uint32_t *blk_cnt;          // [nb] the diff's records per workgroup of 256 buckets, all tables in table order
  uint64_t *blk_off;          // [nb] ... their exclusive scan
  uint32_t nb;                // dint_state_blocks() (0 = blk_cnt / blk_off not allocated)
  unsigned long long *digest_part;  // [DINT_KV_MAX_TABLES][DINT_STATE_DIGEST_GRID][4] the digest's partial per workgroup
};
#define DINT_STATE_DIGEST_GRID 2048u
#define DINT_STATE_WORDS 48u
#define DINT_STATE_DIGEST_AT 16u
uint32_t dint_state_blocks(const dint_kv &kv);
// {rows, sum, xor, 0} of table t into s.words[DINT_STATE_DIGEST_AT + 4 t ..]
void dint_launch_state_digest(const dint_kv &kv, dint_state_scratch s, hipStream_t st);
// what must be done to b's rows to make them a's: the counts into s.words[0..4] and the workgroups' offsets into s.blk_off ...
void dint_launch_state_diff_count(const dint_kv &a, const dint_kv &b, dint_state_scratch s, hipStream_t st);
// ... then (same stream, tables untouched in between) the first `cap` records of the contract's order into d_records
void dint_launch_state_diff_write(const dint_kv &a, const dint_kv &b, dint_state_scratch s, void *d_records, uint64_t cap, hipStream_t st);
// s.words[8] != 0 afterwards: the n records are not grouped by (table, bucket) in ascending order, or name a table that is not there
void dint_launch_state_repair_check(const dint_kv &kv, const void *d_records, uint64_t n, dint_state_scratch s, hipStream_t st);
// s.words[DINT_STATE_HOME_AT] != 0 afterwards: one of the n records (in any order) names a table that is not there or is home to another shard
#define DINT_STATE_HOME_AT 14u
void dint_launch_state_home_check(const dint_kv &kv, const void *d_records, uint64_t n, dint_state_scratch s, hipStream_t st);
// applies the records; emptied overflow entries go to pend set `pend_set` (dint_kv_core.h kv_pool_rotate); counts into s.words[9..12]
void dint_launch_state_repair(const dint_kv &kv, const void *d_records, uint64_t n, uint32_t pend_set, dint_dev_stats *stats,
                              dint_state_scratch s, hipStream_t st);

// ---- table report (k_stats.hip; state_stats.h): occupancy and chain shape, read-only ---------------------------------------
#define DINT_STATE_STATS_GRID 2048u   // workgroups per table at most (8 per compute unit); they stride over the buckets
#define DINT_STATE_STATS_WORDS 80u    // = ST_WORDS = sizeof(dint_table_stats) / 8
struct dint_stats_scratch {
  unsigned long long *part;  // [DINT_KV_MAX_TABLES][DINT_STATE_STATS_GRID][DINT_STATE_STATS_WORDS] one partial report per workgroup
  unsigned long long *out;   // [DINT_KV_MAX_TABLES][DINT_STATE_STATS_WORDS] the tables' reports
};
// table t's report (state_stats.h words; not yet st_report_finish'ed) into s.out[DINT_STATE_STATS_WORDS t ..]
void dint_launch_state_stats(const dint_kv &kv, dint_stats_scratch s, hipStream_t st);

// ---- table verify (k_verify.hip; state_verify.h): the census of chains, lists and pool, and the reclaim of leaked entries ------
#define DINT_STATE_VERIFY_GRID 2048u   // workgroups per table and stage at most; they stride over the buckets / the pool
#define DINT_STATE_VERIFY_WORDS 32u    // = SV_WORDS = sizeof(dint_table_verify) / 8
#define DINT_STATE_VERIFY_PARTS (2u * DINT_STATE_VERIFY_GRID + 1u)  // partial reports of one table: chain stage, the lists, pool stage
struct dint_verify_scratch {
  uint32_t *owner;            // [owner_n] the owner words of every table's pool, table after table (cleared by every call)
  uint64_t owner_n;
  unsigned long long *part;   // [DINT_KV_MAX_TABLES][DINT_STATE_VERIFY_PARTS][DINT_STATE_VERIFY_WORDS]
  unsigned long long *out;    // [DINT_KV_MAX_TABLES][DINT_STATE_VERIFY_WORDS] the tables' reports, then one word the scans' totals go to
  // reclaim only (allocated by the first call that asks for it):
  uint32_t *leaked;           // [owner_n] per table the unaccounted entries ascending
  uint32_t *blk_cnt;          // [blk_n] unaccounted entries per 256 pool entries, table after table
  uint64_t *blk_off;          // [blk_n] ... their exclusive scan, per table
  uint64_t blk_n;
  unsigned long long *heads;  // [DINT_KV_MAX_TABLES][KV_NLISTS] the free lists' head words as they were before the reclaim
};
// tables of kv that the census cannot take (a table of 2^32 - 256 local buckets or more): DINT_EINVAL, else 0
int dint_verify_alloc(const dint_kv &kv, dint_verify_scratch &s, uint32_t flags);
void dint_verify_free(dint_verify_scratch &s);
// table t's words (state_verify.h; not yet sv_report_finish'ed) into s.out[DINT_STATE_VERIFY_WORDS t ..]; with DINT_VERIFY_RECLAIM
// the unaccounted entries are back on the free lists afterwards unless a table's words forbid it.  ev (may be null): four events,
// recorded before the chain stage, behind it, behind the lists, and behind the pool stage and the sum
void dint_launch_state_verify(const dint_kv &kv, dint_verify_scratch s, uint32_t flags, hipStream_t st, hipEvent_t *ev = nullptr);
// ... then the one synchronisation: out[t] finished for every table.  Returns 0, DINT_EHIP, or DINT_ESTATE for a refused reclaim;
// *reclaimed = the entries that went back over all tables
int dint_verify_collect(const dint_kv &kv, dint_verify_scratch s, uint32_t flags, hipStream_t st, struct dint_table_verify *out,
                        uint64_t *reclaimed);

// a dint_tables_view (include/dint_driver.h) checked, then as the launchers and the host forms take tables: no device memory of its
// own.  0, or DINT_EINVAL with dint_last_error set (out: only compared with null)
struct dint_tables_view;
int dint_view_kv(const dint_tables_view *v, const void *out, uint32_t cap_tables, dint_kv *kv);

// ---- table compaction (k_compact.hip; state_compact.h): chains packed, the pool's used part made one range, in place -----------
struct dint_compact_scratch {
  uint32_t *rows = nullptr;              // [sum of n_local] the valid rows of every bucket, table after table
  void *blk_a = nullptr, *blk_b = nullptr;  // [blocks] per 256 buckets {overflow entries afterwards, buckets to rewrite} / {inline entries linked, buckets with a row}
  uint64_t *blk_off = nullptr;           // [blocks] the exclusive scan of the overflow entries, per table
  uint64_t *blk_junk = nullptr;          // [blocks] the second scan's offsets (only its totals are used)
  unsigned long long *sums = nullptr;    // [DINT_KV_MAX_TABLES][4] the four totals of every table
  uint8_t *stage[DINT_KV_MAX_TABLES] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // the staging buffers: stage_cap[t] entries, grown to what a call needs and kept
  uint32_t stage_cap[DINT_KV_MAX_TABLES] = {0, 0, 0, 0, 0};
};
int dint_compact_alloc(const dint_kv &kv, dint_compact_scratch &s);
void dint_compact_free(dint_compact_scratch &s);
// census (vs: dint_verify_alloc'ed), count, scans and -- unless flags has DINT_COMPACT_DRY_RUN -- move and commit, then the one
// synchronisation and out[t] for every table; a staging buffer that is too small is grown (the kernels have done nothing then) and
// the call repeated.  ev (may be null): five events around the four stages.  0, DINT_ESTATE (gate), DINT_ENOMEM, DINT_EHIP
struct dint_table_compact;
int dint_compact_run(const dint_kv &kv, dint_verify_scratch vs, dint_compact_scratch &s, uint32_t flags, hipStream_t st,
                     struct dint_table_compact *out, hipEvent_t *ev);

// ---- block sync (k_block.hip; state_block.h): digests per block of buckets, the blocks that differ, their rows, their diff --------
struct dint_block_scratch {
  unsigned long long *words = nullptr;  // [DINT_BLOCK_WORDS] device words: [0..3] the diff's records by kind, [DINT_BLOCK_TOTAL_AT] the records,
                                        // [DINT_BLOCK_LANES_AT] the buckets of the listed blocks, [DINT_BLOCK_BAD_AT] (u32) state_block.h BK_BAD_*
  unsigned long long *part = nullptr;   // [part_n][4] the digest's partial per chunk of 64 buckets, all tables in table order
  uint64_t part_n = 0;
  uint32_t *id_cnt = nullptr;           // [id_n] buckets of every listed block ...
  uint64_t *id_off = nullptr;           // ... their exclusive scan: a listed block's first lane
  uint64_t id_n = 0;
  uint32_t *blk_cnt = nullptr;          // [blk_n] records per workgroup of 256 lanes ...
  uint64_t *blk_off = nullptr;          // ... their exclusive scan
  uint64_t blk_n = 0;
  uint32_t *run_lo = nullptr, *run_hi = nullptr;  // [run_n] the diff: per lane its bucket's run [lo, hi) in the row list
  uint64_t run_n = 0;
};
#define DINT_BLOCK_WORDS 8u
#define DINT_BLOCK_TOTAL_AT 4u
#define DINT_BLOCK_LANES_AT 5u
#define DINT_BLOCK_BAD_AT 6u
struct dint_block_stats;
bool dint_block_geom(const dint_kv &kv, uint64_t block_buckets, bk_geom *g);  // false: not a block size
uint64_t dint_block_chunks(const dint_kv &kv);
void dint_block_fill_stats(dint_block_stats *out, const bk_geom &g, uint64_t total);
// bk_blocks(g) digests into d_out (s.part: dint_block_chunks(kv) partials, not used for blocks of 64)
void dint_launch_block_digest(const dint_kv &kv, const bk_geom &g, dint_block_scratch s, void *d_out, hipStream_t st);
// n_ids > 0; lanes = an upper bound of the listed blocks' buckets the scratch is sized for (id arrays n_ids, blk arrays lanes / 256
// rounded up, run arrays lanes).  The checks' findings and the totals into s.words ...
void dint_launch_block_rows_count(const dint_kv &kv, const bk_geom &g, const void *d_ids, uint32_t n_ids, uint64_t lanes, dint_block_scratch s, hipStream_t st);
// ... then (same stream, the host has seen no finding) the first `cap` records
void dint_launch_block_rows_write(const dint_kv &kv, const bk_geom &g, const void *d_ids, uint32_t n_ids, uint64_t lanes, dint_block_scratch s, void *d_records,
                                  uint64_t cap, hipStream_t st);
void dint_launch_block_diff_count(const dint_kv &kv, const bk_geom &g, const void *d_ids, uint32_t n_ids, uint64_t lanes, const void *d_rows, uint32_t n_rows,
                                  dint_block_scratch s, hipStream_t st);
void dint_launch_block_diff_write(const dint_kv &kv, const bk_geom &g, const void *d_ids, uint32_t n_ids, uint64_t lanes, const void *d_rows, uint32_t n_rows,
                                  dint_block_scratch s, void *d_records, uint64_t cap, hipStream_t st);

// ---- record routing (k_rroute.hip; state_route.h): a record list partitioned, stably, by home shard of another layout -----------
struct dint_rroute_scratch {
  unsigned long long *words = nullptr;  // [DINT_RROUTE_WORDS] device words: [0] the first record without a home (RR_NO_INDEX: none), [1] the
                                        // scan's total, [2 + h] offsets[h] for h = 0 .. H
  uint32_t *cnt = nullptr;              // [cnt_n] records per (shard, tile), shard-major ...
  uint64_t *off = nullptr;              // ... their exclusive scan: the first output record of every (shard, tile)
  uint64_t cnt_n = 0;
};
#define DINT_RROUTE_WORDS (2u + RR_MAX_SHARDS + 1u)
// n > 0, rr_tiles(n) * g.n_shards <= RR_MAX_COUNTS and <= s.cnt_n.  The check's finding and the offsets into s.words ...
void dint_launch_rroute_count(const rr_geom &g, const void *d_rec, uint64_t n, dint_rroute_scratch s, hipStream_t st);
// ... then (same stream, the host has seen a good list that fits) the n records into d_out
void dint_launch_rroute_write(const rr_geom &g, const void *d_rec, uint64_t n, dint_rroute_scratch s, void *d_out, hipStream_t st);

// ---- held locks (k_locks_state.hip; state_locks.h): the held lock units listed, and released by compare and release ---------------
// the lock units of an engine as the launchers take them (no device memory of its own)
struct dint_locks_view {
  lk_geom g;
  kv_tab tab[DINT_KV_MAX_TABLES];       // kv
  dint_mod lockmod[DINT_KV_MAX_TABLES]; // ... % (4 * hash_size)
  uint2 *tbl;                           // lock tables: the local slots
};
struct dint_locks_scratch {
  unsigned long long *words = nullptr;  // [DINT_LOCKS_WORDS] device words: [0] the first record the list is refused at (LK_NO_INDEX: none), [1] the scan's
                                        // total, [DINT_LOCKS_SUMS_AT + LK_PART r + k] word k of the partials summed over range r (a table)
  uint32_t *cnt = nullptr;              // [nb] held units per workgroup, all tables in table order ...
  uint64_t *off = nullptr;              // ... their exclusive scan
  unsigned long long *part = nullptr;   // [nb][LK_PART] one partial per workgroup (state_locks.h LKS_* / LKU_*)
  uint64_t nb = 0;
};
#define DINT_LOCKS_SUMS_AT 8u
#define DINT_LOCKS_WORDS (DINT_LOCKS_SUMS_AT + LK_PART * LK_MAX_TABLES)
uint64_t dint_locks_blocks(const dint_locks_view &v);       // workgroups of the listing and the sweep
uint64_t dint_locks_list_blocks(uint64_t n);                // ... of the release of a list of n records
// count, scan, sums and -- d_records != nullptr -- the first `cap` records; the totals into s.words
void dint_launch_locks_list(const dint_locks_view &v, dint_locks_scratch s, void *d_records, uint64_t cap, hipStream_t st);
// every held unit released (dry: counted only); the sums into s.words, range = table
void dint_launch_locks_sweep(const dint_locks_view &v, dint_locks_scratch s, bool dry, hipStream_t st);
// n > 0: the list checked (s.words[0]), then -- on the device, only for a list that passed -- compare and release; the sums into range 0
void dint_launch_locks_release(const dint_locks_view &v, dint_locks_scratch s, const void *d_records, uint64_t n, bool dry, hipStream_t st);

// ---- state image (k_image.hip; state_image.h): the tables written out for another shard layout and read back --------
struct dint_image_scratch {
  unsigned long long *words;  // [DINT_IMAGE_WORDS] device words: [2 t] table t's overflow entries, [2 t + 1] its valid slots,
                              // [DINT_IMAGE_BAD_AT] (u32) export: a chain that does not end / check: the SI_BAD_* found
  uint2 *blk;                 // [nb] per workgroup of 256 buckets {overflow entries, valid slots}, all tables in table order
  uint64_t *blk_off;          // [nb] ... the exclusive scan of the entries, per table
  uint32_t nb;                // workgroups blk / blk_off hold
  uint2 *inl;                 // [n_inl] export: the image's {head, next} of every selected inline entry
  uint64_t n_inl;
  uint32_t *ovf_src;          // [n_ovf] export: the pool index of every overflow entry in image order
  uint64_t n_ovf;
};
#define DINT_IMAGE_WORDS 16u
#define DINT_IMAGE_BAD_AT 12u
uint32_t dint_image_blocks(const uint64_t *n, uint32_t n_tables);  // workgroups of 256 for tables of n[t] buckets
bool dint_image_shape(uint32_t workload, uint32_t *n_tables, uint32_t *stride, uint32_t *val_size);
// per table the overflow entries and valid slots of the selected buckets into s.words, the workgroups' offsets into s.blk_off ...
void dint_launch_image_count(const dint_kv &kv, const si_sel *sel, dint_image_scratch s, hipStream_t st);
// ... then (same stream, tables untouched in between) everything behind the header, laid out as h says
void dint_launch_image_write(const dint_kv &kv, const si_sel *sel, const si_header &h, dint_image_scratch s, uint8_t *d_buf, hipStream_t st);
// lock tables: the selected slots to d_slots (nullptr: count only); s.words[1] = the slots with a non-zero word
void dint_launch_image_lock_out(const uint2 *tbl, si_sel sel, uint8_t *d_slots, dint_image_scratch s, hipStream_t st);
void dint_launch_image_check(const si_header &h, const uint8_t *d_buf, bool lock, dint_image_scratch s, hipStream_t st);
// base[t] = the pool entry the image's first overflow entry of table t becomes
void dint_launch_image_import(const dint_kv &kv, const si_header &h, const uint8_t *d_buf, const uint32_t *base, hipStream_t st);
void dint_launch_image_lock_in(uint2 *tbl, uint64_t n_local, const si_header &h, const uint8_t *d_buf, hipStream_t st);
void dint_set_last_error(const char *msg);  // engine.hip: what dint_last_error returns next on this thread

// ---- rehash (k_rehash.hip; state_rehash.h): the rows of a set of engines into a blank engine of another bucket count -----------
struct dint_rehash_scratch {
  unsigned long long *words;  // [DINT_REHASH_WORDS] device words: per table t at [DINT_REHASH_TABLE_WORDS t ..] {rows of the sources,
                              // lock words they hold, the plan's scan total = entries << 32 | overflow entries, rows placed, entries
                              // of the longest chain}; [DINT_REHASH_BAD_AT] (u32) bit 0: a source chain that cannot be walked, bit 1:
                              // a destination bucket beyond SI_MAX_RUN overflow entries
  uint2 *blk;                 // [nb] per workgroup of 256 source buckets {rows, lock words}: table by table, inside a table source by source
  uint64_t *blk_off;          // [nb] ... the exclusive scan of the rows, per table: a workgroup's first row in source order
  uint32_t nb;
  uint32_t *key_in, *head;    // [n_max] one table's unsorted keys / run heads
  uint64_t *loc_in;           // [n_max] ... unsorted locators
  uint64_t n_max;
  uint32_t *key_out, *elist;  // [n_all] every table's sorted keys / first rows of its entries, kept for the build
  uint64_t *loc_out;          // [n_all] ... sorted locators
  unsigned long long *scan;   // [n_all + tables] ... the scan of state_rehash.h (a table's rows + 1 words)
  uint64_t n_all;
  void *tmp;                  // the sort's and the scans' temporary storage
  size_t tmp_bytes;
  const uint8_t **src_entries;  // [DINT_KV_MAX_TABLES][SR_MAX_SRCS] the sources' entries[] by table and source number
};
#define DINT_REHASH_WORDS 48u
#define DINT_REHASH_TABLE_WORDS 8u
#define DINT_REHASH_BAD_AT 40u
uint32_t dint_rehash_blocks(const dint_kv *const *srcs, uint32_t n_srcs);
// per table the sources' rows and held lock words into s.words, the workgroups' offsets into s.blk_off ...
void dint_launch_rehash_count(const dint_kv *const *srcs, uint32_t n_srcs, dint_rehash_scratch s, hipStream_t st);
int64_t dint_rehash_tmp_bytes(uint64_t n, uint64_t dst_n_local, hipStream_t st);
// ... then (same stream, tables untouched in between) table t's keys, sort and plan: blk_at = where its workgroups start in s.blk_off
bool dint_launch_rehash_plan(uint32_t t, const dint_kv *const *srcs, uint32_t n_srcs, uint32_t blk_at, const dint_kv &dst, uint64_t n,
                             uint64_t row_at, dint_rehash_scratch s, hipStream_t st, hipEvent_t *ev);
// ... then (the host has compared every table's need with the destination's pool) the destination's entries
void dint_launch_rehash_build(uint32_t t, const dint_kv &dst, uint64_t n, uint64_t row_at, uint64_t n_ent, uint32_t need,
                              const uint8_t *const *d_src_entries, dint_rehash_scratch s, hipStream_t st);

// ---- bulk load (k_load.hip; state_load.h): rows in insertion order into a table that holds nothing, and the population's rows ----
struct dint_load_scratch {
  unsigned long long *words;  // [DINT_LOAD_WORDS] device words: the foreign rows, the plan's scan total = entries << 32 | overflow entries,
                              // entries of the longest chain, (u32) bit 1: a bucket beyond KV_MAX_CHAIN entries
  uint32_t *key_a, *idx_a;    // [n_max] unsorted keys / row numbers; after the sort the run heads / the buckets' row counts at the run heads
  uint32_t *key_b, *idx_b;    // [n_max] sorted keys / row numbers
  uint32_t *elist;            // [n_max] first rows of the entries
  unsigned long long *scan;   // [n_max + 1] the scan of state_rehash.h
  uint64_t n_max;
  void *tmp;                  // the sort's and the scans' temporary storage
  size_t tmp_bytes;
};
#define DINT_LOAD_WORDS 8u
#define DINT_LOAD_FOREIGN_AT 0u
#define DINT_LOAD_TOTAL_AT 1u
#define DINT_LOAD_LONGEST_AT 2u
#define DINT_LOAD_BAD_AT 4u
int64_t dint_load_tmp_bytes(uint64_t n, uint64_t n_local, hipStream_t st);
void dint_launch_load_count(const dint_kv &kv, uint32_t t, const uint64_t *d_keys, uint64_t n, dint_load_scratch s, hipStream_t st);
bool dint_launch_load_plan(const dint_kv &kv, uint32_t t, const uint64_t *d_keys, uint64_t n, dint_load_scratch s, hipStream_t st, hipEvent_t *ev);
// ... then (the host has compared the need with the pool) the table's entries
void dint_launch_load_build(const dint_kv &kv, uint32_t t, const uint64_t *d_keys, const uint32_t *d_vers, const void *d_vals, uint64_t n, uint64_t n_ent,
                            uint32_t need, dint_load_scratch s, hipStream_t st);
void dint_launch_load_msgs(const dint_kv &kv, uint32_t t, const uint64_t *d_keys, const uint32_t *d_vers, const void *d_vals, uint64_t first, uint32_t m,
                           void *d_req, hipStream_t st);
// the tile table of a data-dependent group (state_load.h SL_G_AI / SL_G_SFCF) for n_subs subscribers, cached per process
int dint_load_tiles(uint32_t group, uint32_t which, uint64_t n_subs, std::vector<uint64_t> *state, std::vector<uint64_t> *rows, uint64_t *total);
void dint_launch_load_gen(uint32_t group, uint32_t which, uint64_t n_subs, const uint64_t *d_tile_state, const uint64_t *d_tile_rows, uint64_t *d_keys,
                          void *d_vals, uint64_t cap, uint32_t val_size, hipStream_t st);

// ---- multi-GPU routing (k_route.hip) --------------------------------------------------------------------------
#define DINT_ROUTE_MAXW 64u        // ranks a batch can be routed to
#define DINT_ROUTE_MAXN 1048576u   // requests per dint_route_pack call
#define DINT_ROUTE_BLK_WORDS (1024u * DINT_ROUTE_MAXW + 64u)  // one copy of the pack kernel's scratch
struct dint_route_scratch {
  uint32_t *blk;       // [1024 tiles][world] requests per tile and destination, then {ticket, words published}: all zero between calls
  uint32_t *blk_next;  // the copy the NEXT call uses (this call zeroes it; the engine swaps the two after every call)
};
// stable partition of n contiguous requests by home rank into `shard.count` slots of `cap` messages, slot w at
// d_send + w * stride, its live count (u32) at d_cnt + w * cnt_stride; d_slot[i] = home * cap + position (or ~0u)
#define DINT_ROUTE_MAXS 4u         // batches (logical servers of one rank) routed by one launch set
struct dint_route_job {            // one batch and the engine whose hash / modulus routes it
  uint32_t workload, msg;
  dint_mod slots;
  const dint_kv *kv;
  dint_shard shard;
  const void *d_req;
  void *d_rep;                     // unpack only
  uint32_t n, cap;
  const uint32_t *d_n;             // live request count on the device (n is then its upper bound), or nullptr
  void *d_send, *d_cnt;            // this batch's slot / live-count word of peer 0
  uint64_t cnt_stride;
  uint32_t *d_slot;
  dint_route_scratch rs;
  dint_dev_stats *stats;
};
void dint_launch_route_pack(const dint_route_job *jobs, uint32_t n_jobs, uint64_t stride, hipStream_t st);
void dint_launch_route_unpack(const dint_route_job *jobs, uint32_t n_jobs, uint64_t stride, hipStream_t st);
