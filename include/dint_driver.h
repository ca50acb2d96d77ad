/*
 * dint_driver.h -- C ABI of the closed-loop transaction drivers (the CALLER of the hot path).
 *
 * The reference's load generators are Caladan programs, one uthread per client, each running
 * complete OCC / 2PL transactions against three replicated shard servers
 * (tatp/caladan/client_udp_shard.cc:177-1185, smallbank/caladan/client_udp_shard.cc:169-1240).
 * They cannot be built here (DPDK / rdma-core / SPDK submodules are not vendored), and no NIC can
 * offer the > 100 M requests/s one MI355X absorbs, so the same transaction state machines are
 * restated here as a deterministic, epoch-synchronous driver:
 *
 *   - W virtual clients, client g seeded 0xdeadbeef + g exactly as ClientLoop does (:1122);
 *   - a transaction is a sequence of PHASES; the messages of one phase are sent together (the
 *     reference sends them from one uthread per shard and joins) and all replies are awaited;
 *   - one EPOCH = every client emits the messages of its current phase; the messages addressed to
 *     shard s (s = key % 3 for reads / locks / primary ops, (s+1)%3 and (s+2)%3 for backups, all three
 *     for logs -- client_udp_shard.cc:187,493-531) form batch s, ordered by client id then send order;
 *     the three shard servers answer; every client consumes its replies and moves on.
 *
 * The driver owns no sockets and no GPU state: the caller carries the batches to the servers
 * (dint_submit of three engines, or the CPU oracle in tests) and hands the replies back.
 */
#ifndef DINT_DRIVER_H
#define DINT_DRIVER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DINT_N_SHARDS 3 /* the reference's deployment: 3 servers, 3-way replication */

typedef struct dint_driver dint_driver_t;

typedef struct dint_driver_config {
  uint32_t workload;      /* DINT_WL_TATP or DINT_WL_SMALLBANK */
  uint32_t n_clients;     /* W */
  uint64_t n_rows;        /* subscribers (tatp) / accounts (smallbank) the keys are drawn from */
  uint32_t first_client;  /* global id of client 0 (seed = 0xdeadbeef + first_client + i) */
  /* key distribution: 0 = the reference's own (tatp_nurand, tatp/caladan/tatp.h:40-43; smallbank hot/cold
   * picker, smallbank.h:30-50); 1 = Zipf(theta) over the rows (BASELINE.json's stress distribution) */
  uint32_t key_dist;
  double zipf_theta;
  uint32_t flags;         /* DINT_DRIVER_*; a bit no flag names: DINT_EINVAL from both *_create calls (was reserved[0]) */
  uint32_t reserved[7];
} dint_driver_config;

/* dint_driver_config.flags.  DINT_DRIVER_LATENCY: the GPU-resident driver keeps the latency histograms below (its emit kernel is
 * then another instantiation, with 2 KB more LDS and a few device atomics per workgroup and epoch); the host driver always keeps
 * its round-trip fields and ignores the flag.  The request stream is the same bytes with and without it. */
#define DINT_DRIVER_LATENCY 1u

typedef struct dint_driver_stats {
  uint64_t txns;          /* finished transactions (committed or not) = the reference's "throughput" count */
  uint64_t committed;     /* = "goodput" */
  uint64_t messages;      /* requests emitted */
  uint64_t by_type[8];    /* finished, per transaction type */
  uint64_t committed_by_type[8];
  uint64_t epochs;
} dint_driver_stats;

int dint_driver_create(const dint_driver_config *cfg, dint_driver_t **out);
void dint_driver_destroy(dint_driver_t *d);
/* wire message size of the driver's workload (55 / 23) */
int dint_driver_msg_size(const dint_driver_t *d);
/* Emit the next epoch.  counts[s] receives the number of messages for shard s; the messages stay in
 * driver-owned buffers returned by dint_driver_batch.  Must alternate with dint_driver_consume. */
int dint_driver_next(dint_driver_t *d, uint32_t counts[DINT_N_SHARDS]);
/* request batch of shard s for the current epoch (valid until the next dint_driver_next) */
const void *dint_driver_batch(dint_driver_t *d, uint32_t shard);
/* hand back the replies (same order, same count as the batches) and advance every client */
int dint_driver_consume(dint_driver_t *d, const void *const replies[DINT_N_SHARDS]);
int dint_driver_get_stats(const dint_driver_t *d, dint_driver_stats *out);

/* ---- transaction latency (dint_amd/csrc/txn_latency.h) ---------------------------------------------------------
 * The reference clients print average, median, 99th and 99.9th percentile latency of COMMITTED transactions beside
 * throughput and goodput (tatp/caladan/client_udp_shard.cc:94-107, :1148-1182; one sample per committed transaction,
 * Percentile() of tatp/caladan/stat.h:12-17).  This is a different quantity from the EPOCH latency of the servers' passes
 * that bench.py reports.  Two measures, per transaction type (the first index: the type numbers of by_type[]):
 *   round trips  r = the epochs in which the transaction emitted messages: it began inside the emit of epoch b, was
 *                finished inside the emit of epoch f, r = f - b.  Histogram index min(r, DINT_LAT_RT_BINS - 1); rt_sum and
 *                rt_max hold r itself (at most 255: the count saturates there).  Both drivers.
 *   ticks        of the device's constant-rate clock, GPU-resident driver only: from the start of the emit kernel of
 *                epoch b to the moment the workgroup that finished the transaction read its clock in epoch f (once per
 *                workgroup, after its clients' phases and their messages).  Log-linear histogram: values below 16 map to
 *                themselves, above that 8 bins per power of two (a bin is at most 12.5 % wide), the last bin saturates at
 *                1.875 * 2^31 ticks (40 s at 100 MHz); dint_latency_tick_lo_host(bin) = the smallest value of a bin.
 *                tick_sum / tick_max hold exact ticks.  A transaction that took more than 31 round trips is timed from
 *                epoch f - 31.
 * aborted_round_trips counts the transactions that did not commit.  That is an extension: the reference samples
 * committed transactions only, and every other field here does the same. */
#define DINT_LAT_RT_BINS 32
#define DINT_LAT_TICK_BINS 240
typedef struct dint_driver_latency {
  uint64_t round_trips[8][DINT_LAT_RT_BINS];         /* committed transactions */
  uint64_t aborted_round_trips[8][DINT_LAT_RT_BINS]; /* the others (extension) */
  uint64_t rt_sum[8], rt_max[8];                     /* committed */
  uint64_t ticks[8][DINT_LAT_TICK_BINS];             /* committed; GPU-resident driver, else 0 */
  uint64_t tick_sum[8], tick_max[8];
  uint64_t tick_khz; /* ticks per millisecond: hipDeviceAttributeWallClockRate.  Where the runtime does not report one, 100000
                      * (the 100 MHz of the CDNA parts' constant clock): ASSUMED then, not read.  0 from the host driver. */
  uint64_t epochs;   /* epochs emitted so far (not reset) */
} dint_driver_latency;
/* round-trip fields and epochs; the tick fields and tick_khz are 0.  Always kept: the host driver has no hot path to protect */
int dint_driver_get_latency(const dint_driver_t *d, dint_driver_latency *out);
/* the tick bin rule on the host, for tests and tools (no device call) */
uint32_t dint_latency_tick_bin_host(uint64_t ticks);
uint64_t dint_latency_tick_lo_host(uint32_t bin); /* bin = DINT_LAT_TICK_BINS: 2^32, where the last bin would end */

/* ---- the same drivers, resident on the GPU -----------------------------------------------
 * Client state lives in HBM; dint_gdriver_next launches a kernel in which every client runs one phase and emits its
 * messages into three driver-owned device arrays -- at exactly the positions, hence with exactly the bytes, of the
 * host driver (tests compare the two streams) -- and writes the three batch sizes to device memory;
 * the shard servers answer IN PLACE (dint_submit_segments(engine_s, dint_gdriver_batch(d, s), 1, cap, cap * msg,
 * counts + s, 0, stream): one segment whose live count the engine reads on the device); dint_gdriver_consume
 * makes every client pick up its replies -- in a kernel of its own, or, when it is issued on the stream of the last
 * dint_gdriver_next (the closed loop), fused into the next emit kernel: the epoch's batches alternate between two buffer
 * sets, so ask dint_gdriver_batch again after every dint_gdriver_next, and keep that stream alive until then.
 * Nothing crosses PCIe.  `cap_per_shard` = slots of each batch array; messages beyond it are dropped and counted
 * (overflow: size it ~1.3x the expected batch). */
typedef struct dint_gdriver dint_gdriver_t;
int dint_gdriver_create(const dint_driver_config *cfg, int32_t device, uint32_t cap_per_shard, dint_gdriver_t **out);
void dint_gdriver_destroy(dint_gdriver_t *g);
int dint_gdriver_next(dint_gdriver_t *g, void *stream);     /* must alternate with dint_gdriver_consume */
int dint_gdriver_consume(dint_gdriver_t *g, void *stream);
void *dint_gdriver_batch(dint_gdriver_t *g, uint32_t shard);  /* device pointer: the CURRENT epoch's cap_per_shard message slots */
const void *dint_gdriver_counts(dint_gdriver_t *g);           /* device pointer: uint32_t[3] live messages per shard */
uint32_t dint_gdriver_cap(const dint_gdriver_t *g);
/* tests / debugging: synchronise and copy the current batch of `shard` to the host; returns its message count */
int64_t dint_gdriver_read_batch(dint_gdriver_t *g, uint32_t shard, void *host, uint64_t cap_msgs);
int dint_gdriver_get_stats(dint_gdriver_t *g, dint_driver_stats *out, uint64_t *overflow);  /* synchronises the device */
/* Transaction latency (struct dint_driver_latency above) of a driver created with DINT_DRIVER_LATENCY; without the flag both
 * calls return DINT_ESTATE.  dint_gdriver_get_latency synchronises the device, like dint_gdriver_get_stats.
 * dint_gdriver_latency_reset zeroes the histograms, sums and maxima in stream order -- the reference's `stat_started` window:
 * issue it on the loop's stream after the warm-up epochs.  The epoch stamps and the clients' round-trip counts are not touched,
 * so a transaction that began before the reset and commits after it is counted with its whole latency. */
int dint_gdriver_get_latency(dint_gdriver_t *g, dint_driver_latency *out);
int dint_gdriver_latency_reset(dint_gdriver_t *g, void *stream);
/* tests / debugging: synchronise and copy the 256 epoch stamps (slot e & 255 = the clock at the start of the emit kernel of epoch
 * e, 0 where no epoch wrote yet) and the number of epochs emitted.  DINT_ESTATE without DINT_DRIVER_LATENCY. */
int dint_gdriver_read_stamps(dint_gdriver_t *g, uint64_t out[256], uint64_t *epochs);

/* ---- lock_fasst load generator ---------------------------------------------------------------------------
 * lock_fasst/caladan/client.cc:183-280 (ClientLoop) over transactions shaped like lock_fasst/caladan/trace_init.sh
 * :6-27, W workers in lock step, one outstanding request each.  dint_fasst_client_next returns the epoch's W 9-byte
 * requests (worker order), dint_fasst_client_consume takes the W replies.  Epochs laid end to end = the request trace
 * (the "24M-op trace": 4096 workers, 24,000,000 keys, read_pct 80, Zipf 0.8 or uniform). */
typedef struct dint_fasst_client dint_fasst_client_t;
typedef struct dint_fasst_client_config {
  uint32_t n_workers;     /* W virtual workers */
  uint32_t first_worker;  /* seed of worker i = 0xdeadbeef + first_worker + i */
  uint32_t key_space;     /* lids are drawn from [0, key_space) */
  uint32_t read_pct;      /* a key of a transaction is read-only with this probability (80) */
  uint32_t key_dist;      /* 0 = uniform (the reference's traces), 1 = Zipf(zipf_theta) */
  uint32_t reserved0;
  double zipf_theta;
  uint32_t reserved[8];
} dint_fasst_client_config;
typedef struct dint_fasst_client_stats {
  uint64_t requests, epochs;
  uint64_t committed;        /* transactions that reached COMMIT (or finished read-only) */
  uint64_t rejects;          /* REJECT_LOCK replies: abort what was locked, restart the transaction */
  uint64_t rollbacks;        /* validation failures: abort every write key, restart */
  uint64_t protocol_errors;  /* a reply the reference client would assert / panic on */
  uint64_t reserved[2];
} dint_fasst_client_stats;
int dint_fasst_client_create(const dint_fasst_client_config *cfg, dint_fasst_client_t **out);
void dint_fasst_client_destroy(dint_fasst_client_t *c);
const void *dint_fasst_client_next(dint_fasst_client_t *c);
int dint_fasst_client_consume(dint_fasst_client_t *c, const void *replies);
int dint_fasst_client_get_stats(const dint_fasst_client_t *c, dint_fasst_client_stats *out);
/* the transaction `worker` is running: keys[0 .. *n_keys) = its sorted read set, wkeys[0 .. *n_wkeys) = its write set (room
 * for 10 each) -- one transaction of lock_fasst/caladan/trace_init.sh's trace files */
int dint_fasst_client_peek(const dint_fasst_client_t *c, uint32_t worker, uint32_t *keys, uint32_t *n_keys, uint32_t *wkeys,
                           uint32_t *n_wkeys);

/* ---- lock_2pl load generator ------------------------------------------------------------------------------
 * lock_2pl/caladan/client.cc:167-240 (ClientLoop) over transactions shaped like lock_2pl/caladan/trace_init.sh:6-27,
 * W workers in lock step, one outstanding request each.  A worker draws its transactions exactly as the lock_fasst
 * worker does (same config: seed 0xdeadbeef + first_worker + i, 5..10 distinct sorted keys, a key is an exclusive lock
 * iff rnd % 100 >= read_pct); it acquires the locks in ascending order, on REJECT with locks held releases them in
 * acquisition order and tries the same transaction again, on REJECT with nothing held sends the same ACQUIRE again, and
 * once every lock is held releases them in reverse order (the transaction has committed).  next / consume as
 * dint_fasst_client_*, 6-byte messages. */
typedef struct dint_tpl_client dint_tpl_client_t;
typedef struct dint_tpl_client_stats {
  uint64_t requests, epochs;
  uint64_t committed;        /* transactions whose locks were all granted (and released) */
  uint64_t rejects;          /* REJECT replies to an ACQUIRE */
  uint64_t protocol_errors;  /* an ACQUIRE answered with neither GRANT nor REJECT, a RELEASE without RELEASE_ACK */
  uint64_t reserved[3];
} dint_tpl_client_stats;
int dint_tpl_client_create(const dint_fasst_client_config *cfg, dint_tpl_client_t **out);
void dint_tpl_client_destroy(dint_tpl_client_t *c);
const void *dint_tpl_client_next(dint_tpl_client_t *c);  /* NULL while the replies of the last epoch are outstanding */
int dint_tpl_client_consume(dint_tpl_client_t *c, const void *replies);
int dint_tpl_client_get_stats(const dint_tpl_client_t *c, dint_tpl_client_stats *out);
/* the transaction `worker` is running: lids[0 .. *n_locks) in ascending order, types[] 1 = exclusive (room for 10 each) */
int dint_tpl_client_peek(const dint_tpl_client_t *c, uint32_t worker, uint32_t *lids, uint8_t *types, uint32_t *n_locks);

/* ---- the lock load generators, resident on the GPU ---------------------------------------
 * The lock_fasst or lock_2pl workers of the host clients above, one lane per worker, state in HBM.  dint_lock_gclient_next
 * launches a kernel in which every worker emits its next request: request i belongs to worker i, so the batch is
 * n_workers messages in worker order -- bit-identical to the host client's.  The lock server answers IN PLACE
 * (dint_submit_device(engine, dint_lock_gclient_batch(c), n_workers, same pointer, stream)); dint_lock_gclient_consume
 * makes every worker take its reply -- in a kernel of its own, or, when issued on the stream of the last
 * dint_lock_gclient_next (the closed loop), fused into the next emit kernel: the epoch's batch alternates between two
 * buffers, so ask dint_lock_gclient_batch again after every next, and keep that stream alive until then
 * (DINT_LOCK_CLIENT_FUSE=0: always a kernel of its own).  Nothing crosses PCIe. */
typedef struct dint_lock_gclient dint_lock_gclient_t;
typedef struct dint_lock_client_config { /* dint_fasst_client_config with the workload where it has reserved0 */
  uint32_t n_workers, first_worker, key_space, read_pct, key_dist;
  uint32_t workload; /* DINT_WL_FASST or DINT_WL_2PL */
  double zipf_theta;
  uint32_t reserved[8];
} dint_lock_client_config;
int dint_lock_gclient_create(const dint_lock_client_config *cfg, int32_t device, dint_lock_gclient_t **out);
void dint_lock_gclient_destroy(dint_lock_gclient_t *c);
int dint_lock_gclient_next(dint_lock_gclient_t *c, void *stream);    /* DINT_ESTATE while the last epoch is not consumed */
int dint_lock_gclient_consume(dint_lock_gclient_t *c, void *stream); /* DINT_ESTATE without a next before it */
void *dint_lock_gclient_batch(dint_lock_gclient_t *c);               /* device pointer: the CURRENT epoch's n_workers messages */
/* tests / debugging: synchronise and copy the current batch (n_workers messages) to the host */
int dint_lock_gclient_read_batch(dint_lock_gclient_t *c, void *host);
/* synchronises the device (a consume deferred into the next emit runs now); rollbacks stay 0 for lock_2pl */
int dint_lock_gclient_get_stats(dint_lock_gclient_t *c, dint_fasst_client_stats *out);

/* ---- log replay: the classification rule on the host (dint_amd/csrc/log_replay.h) --------------------------
 * What dint_log_apply_device (include/dint_abi.h) decides per record on the GPU, restated on the host for tests and tools:
 * records = n canonical 64-byte log records in log order; exists0[i] = does record i's row exist before the whole stream
 * (only read for the first record of a row); types_out[i] = the tatp backup request type dint_amd/recovery.py would
 * choose (COMMIT_BCK 13 / INSERT_BCK 19 / DELETE_BCK 23).  No device call. */
int dint_log_classify_host(const void *records, uint64_t n, const uint8_t *exists0, uint8_t *types_out);

/* ---- log ring: tail words, appended count and drain cursor on the host (dint_amd/csrc/log_ring.h) ----------------
 * What the partition stage of a pass, a kept or cancelled announcement (dint_submit_device_ahead) and dint_log_drain do to the
 * ring of a tatp / smallbank engine of `cap` entries, walked over a script with the functions the engine and the kernels call.
 * ops = n_ops pairs {code, arg}: 0 a plain pass of arg log records; 1 the running pass announces a batch of arg log records;
 * 2 the announced batch is submitted; 3 the announcement is cancelled; 4 a drain into room for arg records.  The ring holds
 * record ids 1, 2, 3 .. in append order (cancelled records included).  After every op four words go to out: {the tail
 * dint_read_log returns, records appended, drain cursor, the other tail word}; a drain adds {n, lost, the n ids}.  Returns the
 * words written; DINT_EINVAL: cap == 0, a null array, arg > cap, an op out of turn, more than out_cap words.  No device call. */
int64_t dint_log_ring_host(uint32_t cap, const uint32_t *ops, uint32_t n_ops, uint64_t *out, uint64_t out_cap);

/* ---- log fold: the rule on the host (dint_amd/csrc/log_fold.h) ---------------------------------------------------
 * What dint_log_apply_folded_device (include/dint_abi.h) decides for ONE chunk, restated over dumped rows for tests and tools:
 * workload = DINT_WL_TATP / DINT_WL_SMALLBANK with n_tables tables of hash_size[t] buckets (dint_hash_size); the replica's rows as
 * dint_dump_rows returns them, table after table: keys / vers [row_off[t] .. row_off[t + 1]) are table t's (dump order is chain
 * order inside a bucket: the first row of a key is the visible one); records = the chunk's n canonical 64-byte log records in
 * log order.  deferred_out[i] = record i goes through the serial replay; repair_out = the repair records in the device call's
 * order, room for cap; out (may be NULL) = applied / commits / inserts / deletes / chunks (1) / rows / folded_records /
 * deferred_records / deferred_buckets / repair_records, the rest zero.  Returns the records written (<= cap; out->repair_records
 * says how many there are), or DINT_EINVAL / DINT_ENOMEM.  No device call. */
struct dint_fold_stats; /* include/dint_abi.h */
int64_t dint_log_fold_host(uint32_t workload, uint32_t n_tables, const uint64_t *hash_size, const uint64_t *row_off,
                           const uint64_t *keys, const uint32_t *vers, const void *records, uint64_t n, uint8_t *deferred_out,
                           void *repair_out, uint64_t cap, struct dint_fold_stats *out);

/* ---- state sync: the rules on the host (dint_amd/csrc/state_sync.h) ------------------------------------------
 * What dint_state_digest / dint_state_diff (include/dint_abi.h) compute on the GPU, restated over dumped rows
 * (dint_dump_rows: keys, versions, values of val_size = 40 or 8 bytes) for tests and tools.  No device call.
 * dint_state_row_hash_host: the hash of one row (0 for a null value or another val_size).
 * dint_state_digest_host: {rows, sum, xr} of n rows of `table`.
 * dint_state_diff_host: rows a and b of ONE table, each in dump order (bucket order is not needed, chain order inside a
 * bucket is what the order of equal-bucket rows is taken for), hash_size = dint_hash_size of the table; the records that make
 * b's visible rows equal a's, in the device call's order; returns how many were written (<= cap), out->total how many there are. */
struct dint_table_digest; /* include/dint_abi.h */
struct dint_diff_stats;
uint64_t dint_state_row_hash_host(uint64_t key, uint32_t ver, uint32_t table, const void *val, uint32_t val_size);
int dint_state_digest_host(uint32_t table, const uint64_t *keys, const uint32_t *vers, const void *vals, uint32_t val_size,
                           uint64_t n, struct dint_table_digest *out);
int64_t dint_state_diff_host(uint32_t table, uint64_t hash_size, uint32_t val_size, const uint64_t *a_keys, const uint32_t *a_vers,
                             const void *a_vals, uint64_t na, const uint64_t *b_keys, const uint32_t *b_vers, const void *b_vals,
                             uint64_t nb, void *records, uint64_t cap, struct dint_diff_stats *out);


/* ---- state image: the check on the host (dint_amd/csrc/state_image.h) ------------------------------------------------
 * The rule dint_state_import (include/dint_abi.h) applies on the GPU before it touches a table, over an image of `bytes` bytes
 * in HOST memory: what a caller runs on a file before uploading it.  Checked: the header against `bytes` and the workload it
 * names, ids strictly ascending, in range and home to the image's source and destination, every link 0, 1 or inside its
 * bucket's run of overflow entries, every chain visiting its run exactly once and in order.  (The match with a particular
 * engine -- n_rows, flags, shard -- is dint_state_import's.)  Returns 0 or DINT_EINVAL; dint_last_error names the first
 * violation.  No device call. */
int dint_state_image_check_host(const void *image, uint64_t bytes);

/* ---- table report: the rule on the host (dint_amd/csrc/state_stats.h) ---------------------------------------------------
 * dint_state_stats (include/dint_abi.h) over a state image of a kv workload in HOST memory: out[t] for every table of the image;
 * returns that number.  The image first goes through dint_state_image_check_host: a malformed one is refused with DINT_EINVAL
 * and nothing is walked; cap_tables smaller than the image's tables: DINT_EINVAL; the image of a lock table: DINT_ESTATE.
 * pool_cap and pool_top are not part of an image and come back 0; longest_chain_bucket is the image's global bucket id.  An
 * engine's OWN image -- (shard_index, shard_count) exported to that same pair -- holds every bucket with chain order, holes
 * and lock words intact, so this report over it equals the device's field for field apart from the two pool words (and from
 * `buckets`, its empty share and histogram bins 0 where a sharded engine's last local bucket lies beyond the table's global
 * size: an image leaves that bucket out).  No device call. */
struct dint_table_stats; /* include/dint_abi.h */
int dint_state_stats_image_host(const void *image, uint64_t bytes, struct dint_table_stats *out, uint32_t cap_tables);

/* ---- held locks: the rule on the host (dint_amd/csrc/state_locks.h) -----------------------------------------------------
 * dint_state_locks (include/dint_abi.h) over a state image in HOST memory: the held units of the image as records[0 .. cap) (any
 * alignment; NULL with cap == 0 only counts), in the call's order, `slot` the local index of the image's SOURCE (src_index,
 * src_count); returns the records written, out->total how many there are.  The image first goes through
 * dint_state_image_check_host: a malformed one is refused with DINT_EINVAL and nothing is walked.  Images of the lock tables are
 * taken (they hold the slots); a store image: DINT_ESTATE.  An engine's OWN image -- (shard_index, shard_count) exported to that
 * same pair -- gives the device's list record for record (but for a sharded engine's last local bucket where it lies beyond the
 * table's global size: an image leaves that bucket out, and it holds no lock).  No device call. */
struct dint_lock_record; /* include/dint_abi.h */
struct dint_lock_stats;
int64_t dint_state_locks_image_host(const void *image, uint64_t bytes, struct dint_lock_record *records, uint64_t cap, struct dint_lock_stats *out);
/* The list check of dint_state_unlock alone, over n records in HOST memory (any alignment): the index of the first record the call
 * would refuse the list at, or n when there is none.  geometry = the engine's: its shard and per table the GLOBAL size (lock tables:
 * n_slots, one table; kv: dint_hash_size of every table).  A workload without lock units has no table: 0 for any n > 0.  No device call. */
struct dint_lock_geometry {
  uint32_t shard_index, shard_count; /* count 0 or 1: unsharded */
  uint32_t n_tables, reserved;
  uint64_t size[5];
};
uint64_t dint_state_unlock_check_host(uint32_t workload, const struct dint_lock_geometry *geometry, const struct dint_lock_record *records, uint64_t n);

/* ---- rehash: the layout rule on the host (dint_amd/csrc/state_rehash.h) -----------------------------------------------
 * Where dint_state_rehash (include/dint_abi.h) puts the rows of ONE table, restated for tests and tools: keys[0 .. n) = the
 * keys of the sources' rows in SOURCE ORDER (the sources' dint_dump_rows, concatenated in srcs order), hash_size = the
 * destination's dint_hash_size of the table, (shard_index, shard_count) = the destination's shard (count 0 or 1: unsharded).
 * Per row i: bucket_out[i] = the destination's local bucket, or UINT64_MAX for a row that is home to another shard (then
 * link_out[i] = 0, slot_out[i] = 0); link_out[i] = the entry that holds the row -- 1 = the bucket's inline entry, k >= 2 = pool
 * entry k - 2 of a destination whose pool was empty; slot_out[i] = 0 .. 3.  Returns the overflow entries the table needs
 * (pool_top afterwards), or DINT_EINVAL (a null array, hash_size 0, shard_index >= shard_count, n > 2^32 - 16) / DINT_ENOMEM.
 * No device call. */
int64_t dint_state_rehash_place_host(const uint64_t *keys, uint64_t n, uint64_t hash_size, uint32_t shard_index, uint32_t shard_count,
                                     uint64_t *bucket_out, uint32_t *link_out, uint32_t *slot_out);

/* ---- table verify: the rule over caller-provided memory (dint_amd/csrc/state_verify.h) ------------------------------------
 * dint_state_verify (include/dint_abi.h) over tables the CALLER describes: what tests and tools use to show the rule a damaged
 * table without a poke into a live engine.  Per table: entries = n_local inline entries followed by pool_cap overflow entries
 * of `stride` bytes (dint_amd/csrc/dint_kv_core.h), hash_size = the table's GLOBAL bucket count (n_local = ceil(hash_size /
 * shard_count)), pool_next[pool_cap], and ctl = DINT_VIEW_CTL_BYTES in the engine's layout: u32 pool_top at 0, u64
 * free_head[64] at 64, u64 pend_head[2][64] behind it.  Both forms check the view before anything else -- workload (store /
 * tatp / smallbank) and table count, stride and value size against the workload's shape, shard_index < shard_count, n_local
 * against hash_size and below 2^32 - 256, pool_cap <= 2^32 - 16, pointers non-null and aligned (entries 16, ctl 8, pool_next
 * 4 bytes) -- and answer DINT_EINVAL to one that fails.  out, cap_tables, flags and the return value are dint_state_verify's.
 * dint_state_verify_view_host: host pointers, no device call.  dint_state_verify_view: device pointers on `device`; the same
 * launchers as the engine call, scratch allocated and freed by the call, one synchronisation of `stream` (NULL: the null stream). */
#define DINT_VIEW_CTL_BYTES 1600u
typedef struct dint_table_view {
  void *entries;
  uint64_t n_local, hash_size;
  uint32_t pool_cap, stride, val_size, reserved;
  uint32_t *pool_next;
  void *ctl;
} dint_table_view;
typedef struct dint_tables_view {
  uint32_t workload, n_tables, shard_index, shard_count;
  dint_table_view table[5];
} dint_tables_view;
struct dint_table_verify; /* include/dint_abi.h */
int dint_state_verify_view_host(const dint_tables_view *view, struct dint_table_verify *out, uint32_t cap_tables, uint32_t flags);
int dint_state_verify_view(int32_t device, const dint_tables_view *view, struct dint_table_verify *out, uint32_t cap_tables,
                           uint32_t flags, void *stream);

/* ---- table compaction: the rule over caller-provided memory (dint_amd/csrc/state_compact.h) ---------------------------------
 * dint_state_compact (include/dint_abi.h) over tables the CALLER describes, with the view and its check of the verify forms
 * above (a view that fails it: DINT_EINVAL).  out, cap_tables, flags (DINT_COMPACT_DRY_RUN) and the return value are
 * dint_state_compact's; a view whose census fails the gate is refused with DINT_ESTATE and not a byte of it changes.
 * dint_state_compact_view_host: host pointers, no device call.  dint_state_compact_view: device pointers on `device`; the same
 * launchers as the engine call, scratch and staging buffer allocated and freed by the call, `stream` (NULL: the null stream)
 * synchronised once per round (two rounds whenever an overflow entry remains: the first sizes the staging buffer). */
struct dint_table_compact; /* include/dint_abi.h */
int dint_state_compact_view_host(const dint_tables_view *view, struct dint_table_compact *out, uint32_t cap_tables, uint32_t flags);
int dint_state_compact_view(int32_t device, const dint_tables_view *view, struct dint_table_compact *out, uint32_t cap_tables,
                            uint32_t flags, void *stream);

/* ---- block sync: the rule over caller-provided memory (dint_amd/csrc/state_block.h) ------------------------------------------
 * dint_state_block_digest / dint_state_block_rows / dint_state_block_diff (include/dint_abi.h) over tables the CALLER describes in
 * HOST memory, with the view and its check of the verify forms above (a view that fails it: DINT_EINVAL).  Digests, ids, rows and
 * records are host memory (rows and records at any alignment); arguments, order, refusals and return values are the device calls'.  A refused call
 * writes not a byte.  No device call. */
struct dint_block_digest; /* include/dint_abi.h */
struct dint_block_stats;
int64_t dint_state_block_digest_host(const dint_tables_view *view, uint64_t block_buckets, struct dint_block_digest *out, uint64_t cap_blocks,
                                     struct dint_block_stats *out_stats);
int64_t dint_state_block_rows_host(const dint_tables_view *view, uint64_t block_buckets, const uint32_t *ids, uint32_t n_ids, void *records,
                                   uint64_t cap, struct dint_block_stats *out_stats);
int64_t dint_state_block_diff_host(const dint_tables_view *view, uint64_t block_buckets, const uint32_t *ids, uint32_t n_ids, const void *rows,
                                   uint64_t n_rows, void *records, uint64_t cap, struct dint_diff_stats *out_stats);

/* ---- bulk load: the rule over caller-provided memory (dint_amd/csrc/state_load.h) -----------------------------------------------
 * dint_state_load_place_host: the direct load of dint_load_rows_device (include/dint_abi.h) into table `table` of a view in HOST
 * memory (the view and its check of the verify forms above), which must hold nothing: keys / vers (may be NULL) / vals[n][val_size]
 * in insertion order.  Return value, refusals (DINT_ENOMEM, DINT_ESTATE: not a byte written) and `out` are the device call's.
 * dint_populate_rows_host: the rows that subscribers / accounts first .. first + count - 1 add to `table` of the reference's
 * population of `workload`, in insertion order, through the rule the generation kernels run; returns their number (also when it
 * exceeds cap: only cap rows are written), or DINT_EINVAL.  vals: 40 bytes per row, 8 for smallbank.
 * dint_populate_tile: subscribers per workgroup of the generation kernels.  dint_populate_tile_states_host: the tile table of a
 * data-dependent table (tatp 2, 3, 4; any other: DINT_ESTATE) for n_subs subscribers -- state[k] = fastrand's state at subscriber
 * k * tile, rows[k] = the table's rows of the subscribers before it, k = 0 .. n_subs / tile; returns the entries (only cap are
 * written).  The table is computed once per process and continued to the largest n seen.  No device call in any of them. */
struct dint_load_stats; /* include/dint_abi.h */
int dint_state_load_place_host(const dint_tables_view *view, uint32_t table, const uint64_t *keys, const uint32_t *vers, const void *vals,
                               uint64_t n, struct dint_load_stats *out);
int64_t dint_populate_rows_host(uint32_t workload, uint32_t table, uint64_t first, uint64_t count, uint64_t *keys, void *vals, uint64_t cap);
uint32_t dint_populate_tile(void);
int64_t dint_populate_tile_states_host(uint32_t workload, uint32_t table, uint64_t n_subs, uint64_t *state, uint64_t *rows, uint64_t cap);

/* ---- record routing: the rule over caller-provided memory (dint_amd/csrc/state_route.h) ----------------------------------------
 * dint_records_route (include/dint_abi.h) over a list in HOST memory, at any alignment: the stable partition of the n 64-byte records
 * at rec by home shard -- (fasthash64(key) % the table's bucket count) % dst_count, the bucket counts those of an engine of
 * `workload` (store / tatp / smallbank; anything else DINT_ESTATE) created with n_rows -- into out (room for n records), and the
 * dst_count + 1 offsets.  Returns n.  dst_count 0 or above 255, a missing buffer, input and output overlapping, a record whose table
 * the workload has not (dint_last_error names the first): DINT_EINVAL, with neither out nor offsets written.  No device call. */
int64_t dint_records_route_host(uint32_t workload, uint64_t n_rows, uint32_t dst_count, const void *rec, uint64_t n, void *out,
                                uint64_t *offsets);
/* records per workgroup of dint_records_route's kernels: the sizes at which the device path changes shape (one tile, two, ...) */
uint32_t dint_records_route_tile(void);

/* ---- traffic report: the rule over caller-provided memory (dint_amd/csrc/traffic_report.h) -------------------------------------
 * dint_traffic_report (include/dint_abi.h) over a batch in HOST memory, at any alignment: reqs / replies (may be NULL) = n wire
 * messages of `workload`; the geometry is that of an engine created with (workload, n_slots, n_rows, flags) -- lock tables n_slots
 * (0: the reference's 36,000,000), kv workloads the bucket counts dint_engine_create derives from n_rows, through the function it
 * derives them with (no dint_config flag changes a bucket count today; `flags` is handed to that function so that one that does is
 * followed here too).  out, the two lists (top_k entries each), their order and every refusal are the device call's; temp_bytes
 * is 0.  A refused call writes nothing.  No device call. */
struct dint_traffic_report; /* include/dint_abi.h */
struct dint_traffic_key;
int dint_traffic_report_host(uint32_t workload, uint64_t n_slots, uint64_t n_rows, uint32_t flags, const void *reqs, const void *replies,
                             uint64_t n, uint32_t top_k, struct dint_traffic_report *out, struct dint_traffic_key *by_requests,
                             struct dint_traffic_key *by_rejects);

#ifdef __cplusplus
}
#endif
#endif /* DINT_DRIVER_H */
