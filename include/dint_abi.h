/*
 * dint_abi.h -- C ABI of the MI355X batched transaction-certification engine.
 *
 * This is the drop-in boundary for ONE path of DINT: the per-packet server state
 * machine (lock_fasst / lock_2pl lock tables, store KV, log append, TATP and
 * SmallBank shard servers).  The reference has no function API for this path --
 * its boundary is the UDP wire protocol (one packed request struct per datagram,
 * the reply is the same struct mutated in place) -- so the ABI is the *batched form
 * of the reference's handler loop*:
 *
 *   reference (one message at a time)                      this ABI (N messages)
 *   -----------------------------------------------------  ----------------------------
 *   lock_fasst/udp/server.cc:78-119   server_loop body     dint_submit(workload FASST)
 *   lock_2pl/udp/server.cc:70-122     server_loop body     dint_submit(workload 2PL)
 *   log_server/udp/server.cc:73-88    server_handler body  dint_submit(workload LOG)
 *   store/udp/server.cc:72-98         server_handler body  dint_submit(workload STORE)
 *   tatp/udp/server_shard.cc:113-210  server_handler body  dint_submit(workload TATP)
 *   smallbank/udp/server_shard.cc:107-189                  dint_submit(workload SMALLBANK)
 *   (eBPF flavour: lock_fasst/ebpf/ls_kern.c:32-100 ls_xdp_main and siblings)
 *
 * Contract (SURVEY.md 8 "parity target"): for a request array R[0..n) the reply
 * array and the final table/log state equal those of the reference udp/ server
 * processing R in index order on one thread.  reqs/replies are arrays of the exact
 * `#pragma pack(1)` wire structs (9 / 6 / 53 / 53 / 55 / 23 bytes, see dint_msg_size);
 * replies[i] answers reqs[i]; every byte the reference does not overwrite is echoed.
 * Per-request errors never abort a batch: an unknown type/table leaves the reply
 * equal to the request and is counted in dint_stats (the reference would panic()).
 *
 * No torch/HIP types appear in any signature: device pointers and the stream are
 * passed as void*.  All functions return 0 or a negative DINT_E* code.
 */
#ifndef DINT_ABI_H
#define DINT_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DINT_ABI_VERSION 5 /* v4 (round 6): dint_submit_device_ahead, dint_stats.late_requests; v5: dint_log_drain_device,
                              dint_log_apply_device */

/* dint_config.flags */
#define DINT_FLAG_KV_ROUNDS 1u /* kv workloads: resolve same-key conflicts request by request instead of in
                                  closed form (slow; identical results -- used for A/B runs and parity tests) */

#define DINT_FLAG_COPY_STREAMS 2u /* host path: dedicated H2D / D2H streams, so that one engine overlaps the copies of
                                     neighbouring passes with its kernels.  Off by default: a process that runs several
                                     engines has them overlap each other, and every extra stream beyond HIP's hardware
                                     queues (GPU_MAX_HW_QUEUES, 4) can serialise two engines behind one queue */

#define DINT_FLAG_LOCK_SAME_KEY 4u /* tatp: the eBPF ablation build tatp/ebpf/lock_kern.c -- a lock slot remembers the key it
                                     was granted to and a rejected ACQUIRE_LOCK for that same key is answered
                                     REJECT_LOCK_SAME_KEY (28) instead of REJECT_LOCK (:289-298; counted by
                                     tatp/caladan/client_lock.cc:762-771 to tell true conflicts from slot aliasing).
                                     Diagnostic: requests are resolved one by one (as DINT_FLAG_KV_ROUNDS) */

#define DINT_FLAG_KV_NO_HOT 8u /* kv workloads: big bins never take the dominant-key path (A/B runs; identical results) */

#define DINT_FLAG_INPUTS_READY 16u /* lock tables, dint_submit_device only.  The caller promises that (1) the request bytes of a
                                      batch are in device memory when the call is made -- not produced by work still
                                      pending on `stream` --, and (2) the request / reply buffers of a call do not overlap
                                      the buffers of EARLIER calls whose replies have not been consumed yet.  The engine
                                      then runs the first half of a pass (classify, hash, bin the requests: it touches
                                      no table) on a stream of its own beside the second half of the previous pass;
                                      replies still complete in the order of the calls on `stream`, and the table is
                                      still updated batch after batch.  A receive ring that is filled by a copy engine
                                      and handed over when complete -- what the reference's recv loop does with its
                                      socket buffer (lock_fasst/udp/net.h:33-48) -- satisfies both.  Without the flag a
                                      call is fully stream-ordered (the default).  Memory: the first piped call allocates two
                                      more sets of pass scratch, ~0.5 GB of address space each (touched as filled).  The kv
                                      workloads' form of the promise is per call: dint_submit_device_ahead */

#define DINT_FLAG_SHARD_REPLICA 0x20u /* (= 32) store / tatp / smallbank engines with shard_count > 1: the engine is one shard of a REPLICA
                                         set and takes what writes to a replica -- dint_state_repair, dint_state_diff (against the
                                         same shard of another set), dint_log_apply_device and dint_log_apply_folded_device -- over
                                         records that dint_records_route brought to its layout: a record is placed at its LOCAL
                                         bucket, and a list that holds a record of another shard is refused whole.  Without the flag
                                         a sharded engine refuses these calls, as it always has; an unsharded engine ignores it.
                                         The request path, the block sync and every other call are the same either way */

/* workloads (dint_config.workload) */
enum {
  DINT_WL_FASST = 0,     /* lock_fasst: 9-byte {u8 type; u32 lid; u32 ver}            net.h:23-29 */
  DINT_WL_2PL = 1,       /* lock_2pl:   6-byte {u8 action; u32 lid; u8 type}          net.h:25-31 */
  DINT_WL_LOG = 2,       /* log_server: 53-byte {u8 type; u64 key; u8 val[40]; u32 ver}           */
  DINT_WL_STORE = 3,     /* store:      53-byte, same layout.  READ / SET are store/udp/server.cc:75-97; INSERT
                            (type 2 -> 8) is an ENGINE EXTENSION with kvs_insert semantics and no reference parity
                            target: store/udp panics on it and store/ebpf's type 2 is a cache fill */
  DINT_WL_TATP = 4,      /* tatp:       55-byte {u8 ord,type,table; u64 key; u8 val[40]; u32 ver} */
  DINT_WL_SMALLBANK = 5, /* smallbank:  23-byte {u8 ord,type,table; u64 key; u8 val[8]; u32 ver};
                            the udp server's 7 request types + WARMUP_READ (17 -> 18) of the eBPF flavour */
  DINT_WL_COUNT = 6
};

/* error codes */
enum {
  DINT_OK = 0,
  DINT_EINVAL = -1,   /* bad argument / unsupported configuration */
  DINT_ENOMEM = -2,   /* host or device allocation failed */
  DINT_EHIP = -3,     /* a HIP runtime call failed (see dint_last_error) */
  DINT_ENODEV = -4,   /* no usable gfx950 device */
  DINT_ESTATE = -5    /* call not valid for this engine's workload */
};

/* The largest request count one kernel pass handles: dint_submit splits larger
 * arrays into consecutive passes (correct by the serial-order contract).  DINT_KV_PASS_MAX for every
 * workload (see max_pass), never more than the log ring holds (log_server, tatp, smallbank); DINT_MICRO_BATCH was the
 * log_server limit until r03 and remains as the batch size of BASELINE's micro configs. */
#define DINT_MICRO_BATCH 65536u
#define DINT_KV_PASS_MAX 1048576u

typedef struct dint_config {
  uint32_t abi_version;  /* DINT_ABI_VERSION */
  uint32_t workload;     /* DINT_WL_* */
  int32_t device;        /* HIP device ordinal; -1 = current device */
  uint32_t flags;        /* DINT_FLAG_* */
  /* FASST / 2PL: number of lock slots; slot = fasthash64(lid,4,0xdeadbeef) % n_slots.
   * 0 = the reference's 36,000,000 (lock_fasst/udp/utils.h:12). */
  uint64_t n_slots;
  /* STORE: subscribers (buckets = n_rows*18/4, store/udp/server.cc:112-114; 0 = 2,000,000)
   * TATP : subscribers (bucket counts per tatp/udp/server_shard.cc:75-79; 0 = 7,000,000)
   * SMALLBANK: accounts (buckets = n_rows*3/2/4, smallbank/udp/server_shard.cc:75-76; 0 = 24,000,000) */
  uint64_t n_rows;
  /* log ring entries (LOG/TATP/SMALLBANK); 0 = the reference's 1,000,000 */
  uint32_t log_entries;
  /* multi-GPU hash sharding: this engine owns global slots/buckets g
   * with g % shard_count == shard_index and stores them at g / shard_count.  Requests
   * handed to dint_submit must already be routed to their home shard (dint_home_shard).
   * shard_count 0 or 1 = unsharded. */
  uint32_t shard_index;
  uint32_t shard_count;
  /* requests per kernel pass; longer submissions run as several passes.  0 = the engine's default: 1,048,576 (LOG / TATP /
   * SMALLBANK never more than log_entries), FASST / 2PL 65,536 (BASELINE's batch size: the lock kernels' hot-slot path
   * covers passes up to that; a longer pass is legal -- ask for it here -- and slower per request on skewed streams). */
  uint32_t max_pass;
  /* STORE / TATP / SMALLBANK: overflow entries per table (a bucket whose 4 inline slots are taken chains 4-slot
   * entries from this pool; the reference `new`s them without bound, store/udp/kvs.h:95-102).  0 = local buckets / 4
   * + 4096 (twice what the reference population needs).  A full pool refuses INSERTs: see dint_stats.pool_exhausted. */
  uint32_t pool_entries;
  uint32_t reserved[3];
} dint_config;

typedef struct dint_stats {
  uint64_t batches;        /* micro-batches processed */
  uint64_t requests;       /* requests processed */
  uint64_t bad_requests;   /* unknown type / table: reply left equal to request */
  uint64_t missing_keys;   /* SET/COMMIT/DELETE (tatp) or lock+read (smallbank) on a missing key:
                              the reference panics (tatp/udp/kvs.h:91,152); ack still sent */
  uint64_t foreign_requests; /* request whose home shard is not this engine: left untouched */
  uint64_t pool_exhausted; /* INSERTs that found the overflow-entry pool full: nothing is stored; a request resolved on
                              its own is answered REJECT_INSERT (store, 9) / REJECT_COMMIT (tatp, 11 -- the eBPF
                              flavour's "refused, send again", tatp/ebpf/shard_kern.c:509-514) -- every one: a bucket
                              run that inserts leaves the closed forms while the pass's INSERTs could use the pool up;
                              dint_wait / dint_submit / dint_sync return DINT_ENOMEM */
  uint64_t route_overflow; /* requests dint_route_pack could not place (destination slot full): answered by
                              dint_route_unpack with the back-pressure reply of dint_refuse ("not now, send again") */
  uint64_t big_bin_requests; /* kv workloads: requests that were resolved by the big-bin kernel (hot keys) */
  uint64_t late_requests;  /* store / tatp (ABI v4): requests of hot subs that no closed form of k_kv_hot covered and the general
                              path answered (k_kv_late) -- a diagnostic: they are the slow ones.  smallbank: requests of subs whose
                              row the pieces refused (kv_sb_item: more than 512 requests or more than 8 foreign ones in a piece,
                              an unknown op) and one workgroup answered the old way */
  uint64_t reserved[3];    /* [0..2] (v4): the late work items by kind -- store / tatp {sub as listed, solo, pieces}; smallbank: why a
                              row was refused {a piece over 512 requests, over 8 foreign requests, an unknown op} */
} dint_stats;

typedef struct dint_engine dint_engine_t;

/* ---- lifecycle ---------------------------------------------------------- */
int dint_engine_create(const dint_config *cfg, dint_engine_t **out);
void dint_engine_destroy(dint_engine_t *e);
/* bytes of one wire message of `workload` (9/6/53/53/55/23), or DINT_EINVAL */
int dint_msg_size(uint32_t workload);
/* human-readable text of the last failure on this thread */
const char *dint_last_error(void);

/* ---- the hot path -------------------------------------------------------- */
/* Host buffers: copies reqs to the GPU, runs the batch, copies replies back;
 * returns when replies are complete.  reqs == replies (in place) is allowed.
 * = dint_submit_async + dint_wait. */
int dint_submit(dint_engine_t *e, const void *reqs, uint32_t n, void *replies);
/* Pipelined form: enqueue and return at once; *ticket identifies the submission.  The array is cut
 * into passes of max_pass requests; pass k+1's host-to-device copy and pass k-1's device-to-host copy overlap pass
 * k's kernels (DINT_FLAG_COPY_STREAMS: three HIP streams; three staging slots), and successive submissions pipeline the same way -- as long
 * as reqs / replies are page-locked (dint_alloc_pinned, or the caller's own hipHostMalloc / hipHostRegister
 * memory).  Pageable buffers (plain malloc memory, as the reference's stack `message` of lock_fasst/udp/net.h:33-48) work
 * too: the engine stages them through page-locked buffers of its own -- one host memcpy on submission, and the replies
 * reach the caller's buffer inside dint_wait -- so the HIP runtime is never handed pageable memory.  Buffers must stay
 * untouched until dint_wait(ticket) returns; replies are valid only then.  Submissions are applied in call order (one
 * serial history per engine). */
typedef uint64_t dint_ticket;
int dint_submit_async(dint_engine_t *e, const void *reqs, uint32_t n, void *replies, dint_ticket *ticket);
/* replies of `ticket` (and of every earlier ticket) are complete.  DINT_ENOMEM if INSERTs were refused since the
 * last check (dint_stats.pool_exhausted) -- the replies are valid, rows were not stored.  Every refusal is reported once: a
 * dint_sync between the submission and its dint_wait takes the report, and the dint_wait then returns 0.  Refusals of
 * dint_submit_device batches on a caller's stream are reported by the first dint_wait / dint_sync after they have run. */
int dint_wait(dint_engine_t *e, dint_ticket ticket);
int dint_alloc_pinned(size_t bytes, void **out);
void dint_free_pinned(void *p);
/* Device buffers (HBM-resident, e.g. torch tensors): enqueues the batch on `stream`
 * (a hipStream_t, NULL = the engine's own stream) and returns immediately; in-place
 * allowed.  Buffers must stay valid until the stream reaches the end of the batch.
 * Stream rule: an engine has ONE set of batch scratch, so its passes run one after the other.  When consecutive
 * calls (submit, load, populate, route) name different streams the engine inserts the event wait itself; work the
 * CALLER enqueues on other streams (producing d_reqs, consuming d_replies) is the caller's to order --
 * dint_stream_wait / dint_stream_signal do that for the engine's own stream. */
int dint_submit_device(dint_engine_t *e, const void *d_reqs, uint32_t n, void *d_replies, void *stream);
/* The same with a LOOK-AHEAD (round 6; store / tatp / smallbank / lock_fasst / lock_2pl -- log_server ignores the announcement): (d_next_reqs, next_n,
 * d_next_replies) is the batch of the engine's NEXT dint_submit_device[_ahead] call.  The caller promises that (1) that call
 * will be made, with exactly these pointers and this count, before anything else is submitted to the engine, (2) the
 * batch's request bytes are complete in device memory in the order of `stream` -- produced by work enqueued on `stream`
 * before THIS call, or simply there: a receive ring the NIC has filled, as the reference's recv loop finds a whole
 * `message` in its socket buffer before the switch runs (tatp/udp/server_shard.cc:110-114) --, and (3) its buffers do not
 * overlap this call's.  The engine then runs the next batch's table-free first stage (classify, hash, partition into the
 * pass's coarse bins, and the log appends of its COMMIT_LOG / DELETE_LOG requests) in the SAME kernel launch as this batch's
 * hot keys (k_kv_hot_part) and starts the next call at its resolve kernel: a pass's chain is two launches instead of four.
 * Replies, table state and log ring are exactly those of two plain calls.
 * Between the two calls (tatp / smallbank): the ring holds the announced batch's log records already, and dint_log_drain /
 * dint_log_drain_device hand them out with the rest; the tail dint_read_log returns does NOT include them yet (it is the ring
 * position behind the batches that were answered).
 * A BROKEN announcement -- a different next submission, or a launch set that does not match
 * (dint_submit_segments_multi_ahead) -- fails with DINT_ESTATE and answers nothing; dint_snapshot and the state calls fail
 * with DINT_ESTATE and leave the announcement pending.  After a broken announcement the engine is as if it had never seen the
 * announced batch: tables, lock words and overflow pool (the first stage never touches them), the ring's tail and the count of
 * records appended, dint_stats (bad_requests / foreign_requests the first stage counted are taken back; lock_fasst / lock_2pl:
 * those two counters keep what the cancelled count stage added), and the drain cursor.  One thing stays: the ring slots from
 * the tail onward hold the cancelled batch's log records, as many as it had log requests.  Nothing reads them as records, but
 * a later tatp DELETE_LOG that lands on such a slot keeps the 40 val bytes it finds there (the reference's DELETE_LOG writes no
 * val, tatp/udp/server_shard.cc:196-207), so it shows the cancelled batch's bytes where two plain calls would show older ones.
 * Records drained between the two calls and then cancelled are the caller's to discard; the drain stream after the cancel goes
 * on with the first record appended after it: nothing lost, nothing repeated, lost == 0.  (A cancelled batch that lapped the
 * reader -- more records waiting to be drained plus its own than the ring holds -- has overwritten the oldest of them: the
 * next drain reports those as lost, like any record the ring overwrote.)  The announced batch's reply buffer (= its request
 * buffer, when in place) holds what the first stage wrote: undefined for the caller.
 * dint_reset / dint_restore drop the announcement silently: the engine goes on as a fresh one / from the snapshot (ring, tail,
 * drain cursor included).  lock_fasst / lock_2pl (batches of at most 65,536): the count
 * stage of the next batch rides in this batch's resolve launch the same way (k_lock_pass); an engine with
 * DINT_FLAG_INPUTS_READY takes an announcement only in a pass it does not pipe (kernel timing on) and ignores it otherwise.
 * A dint_submit_device of more requests than one pass takes looks
 * ahead from pass to pass by itself (stream order already has the whole array complete). */
int dint_submit_device_ahead(dint_engine_t *e, const void *d_reqs, uint32_t n, void *d_replies, const void *d_next_reqs,
                             uint32_t next_n, void *d_next_replies, void *stream);
/* wait for everything enqueued on the engine's own streams; replies of dint_submit_async calls from pageable memory that are
 * still staged in the engine's page-locked buffers reach the caller's buffers here too (as in dint_wait).  store / tatp:
 * DINT_ENOMEM if INSERTs -- of dint_submit_device batches on the engine's own stream, which no dint_wait sees -- were refused
 * since the last check (dint_stats.pool_exhausted); everything is complete and the replies are valid also then. */
int dint_sync(dint_engine_t *e);
/* the engine's own stream (a hipStream_t) */
void *dint_engine_stream(dint_engine_t *e);
/* requests one kernel pass takes (dint_config.max_pass after clamping) */
uint32_t dint_max_pass(dint_engine_t *e);
/* the engine's own stream waits for everything enqueued so far on other_stream / other_stream waits for the engine */
int dint_stream_wait(dint_engine_t *e, void *other_stream);
int dint_stream_signal(dint_engine_t *e, void *other_stream);

/* Back-pressure: the reply the reference's eBPF servers give when they cannot take a request right
 * now -- REJECT_READ / REJECT_LOCK / REJECT_COMMIT (tatp), RETRY (smallbank, lock_2pl), kReject* (store) -- which every
 * client answers by sending the request again (e.g. tatp/caladan/client_ebpf_shard.cc:434-442).  A front end that must
 * shed load (the UDP shim with its submission queue full) fills replies with this instead of queueing; no GPU work,
 * no state change.  Request types that the eBPF servers never refuse are left as they are (= not answered). */
int dint_refuse(uint32_t workload, const void *reqs, uint32_t n, void *replies);

/* ---- population / state (parity + checkpointing) -------------------------- */
/* KV workloads: bulk-insert rows in order with kvs_insert semantics (ver given, or 0 if
 * vers == NULL).  val_size is 40 (store/tatp) or 8 (smallbank).  Host pointers. */
int dint_load_rows(dint_engine_t *e, uint32_t table, const uint64_t *keys, const uint32_t *vers,
                   const void *vals, uint64_t n);
/* generate and load the reference's initial population for the first `populate_n`
 * subscribers/accounts (store/udp/tatp.h:44-66, tatp/udp/tatp.h:283-412,
 * smallbank/udp/smallbank.h:105-127); value structs are zero-initialised first. */
int dint_populate(dint_engine_t *e, uint64_t populate_n);
/* number of buckets of `table` (global, before sharding) */
int64_t dint_hash_size(dint_engine_t *e, uint32_t table);
/* dump all valid rows of `table` (bucket order, chain order inside a bucket);
 * returns the row count (also when it exceeds cap; only cap rows are written). */
int64_t dint_dump_rows(dint_engine_t *e, uint32_t table, uint64_t *keys, uint32_t *vers, void *vals,
                       uint64_t cap);
/* lock-word state, one u32 per LOCAL lock slot:
 *   FASST: a=lock (0/1), b=version        2PL/SMALLBANK: a=num_ex, b=num_sh
 *   TATP : a=txn lock (0/1), b=0 (b may be NULL)
 * FASST/2PL: n = ceil(n_slots / shard_count) words, index = global slot / shard_count.
 * TATP/SMALLBANK (`table` selects the table): n = 4 * local buckets, index = q * n_local + local bucket with
 * q = lock_hash / hash_size -- i.e. exactly lock_hash (tatp/udp/tatp.h:12-14) when unsharded.
 * Returns n (also when cap is smaller; only cap words are written). */
int64_t dint_read_locks(dint_engine_t *e, uint32_t table, uint32_t *a, uint32_t *b, uint64_t cap);
/* log ring: copies up to cap canonical 64-byte records
 * {u64 key; u8 val[40]; u32 ver; u8 is_del; u8 table; u8 pad[10]} and returns the tail index: the ring position behind the
 * batches answered so far (a batch announced by dint_submit_device_ahead has its records in the ring, from the tail on, but is
 * not counted into the tail before it is submitted) */
int64_t dint_read_log(dint_engine_t *e, void *records, uint64_t cap);
/* Log drain (the reference writes its logs and never reads them, tatp/udp/server_shard.cc:182-207): copies
 * the records appended since the previous call, oldest first, up to cap; returns how many.  *lost (may be NULL) = records
 * the ring overwrote before they were drained (drain at least once per log_entries appended).  The stream position
 * survives ring wrap-around; dint_reset rewinds it.  dint_amd/recovery.py replays a drained log into a replica.
 * dint_log_drain_device / dint_log_apply_device below are the same two steps without the trip through host memory. */
int64_t dint_log_drain(dint_engine_t *e, void *records, uint64_t cap, uint64_t *lost);
/* (ABI v5) like dint_log_drain, but the records go to DEVICE memory (64-byte canonical records, oldest first): d_records is
 * readable and writable from the engine's device.  Shares dint_log_drain's cursor, its `lost` accounting and its contract
 * (ring wrap, reset / restore) -- the two calls may be mixed.  The copy runs on `stream` (a hipStream_t, NULL = the engine's
 * own) and is complete when the call returns: like dint_log_drain it synchronises the device to learn the tail; the 16 bytes of
 * the tail words are all that reaches host memory.  As for dint_log_drain, a batch announced by dint_submit_device_ahead has
 * its records in the ring already: they are drained with the rest (and are the caller's to discard should the announcement be
 * broken: the cursor then goes back behind the last answered batch's records). */
int64_t dint_log_drain_device(dint_engine_t *e, void *d_records, uint64_t cap, uint64_t *lost, void *stream);

typedef struct dint_apply_stats {
  uint64_t applied, commits, inserts, deletes; /* records turned into COMMIT_BCK / INSERT_BCK / DELETE_BCK and acked */
  uint64_t chunks;                             /* passes the stream was cut into */
  uint64_t reserved[3]; /* diagnostic, with dint_timing_enable on: nanoseconds on the engine's stream spent in [0] the key pass
                           and the sort, [1] the probe (build, READ pass, classify, emit), [2] the apply pass and the count */
} dint_apply_stats;

/* (ABI v5) replay n drained records (device pointer, log order) into engine e through its ordinary hot path:
 * tatp: COMMIT_BCK for a row that exists at that point of the log, INSERT_BCK for one that does not,
 *       DELETE_BCK for a DELETE_LOG record;  smallbank: COMMIT_BCK, val = the record's first 8 bytes.
 * chunk = records per pass, 0 = dint_max_pass(e) (larger values are clamped to it).  Everything is enqueued on the engine's
 * own stream, which must already be ordered behind whatever produced the records (dint_log_drain_device returns with them
 * complete; dint_stream_wait otherwise).  Returns when the work is queued unless out != NULL, which synchronises the stream
 * and fills the counts.  The records stay untouched.  Refused before any GPU work: a workload without a KV log target
 * (DINT_ESTATE), a sharded engine without DINT_FLAG_SHARD_REPLICA (DINT_EINVAL: the log must be routed first), a batch announced by
 * dint_submit_device_ahead still pending (DINT_ESTATE, as dint_snapshot).  The replica's own log is not appended to (backup
 * operations never are).  Scratch of ~200 bytes per record of a chunk is allocated on the first call and kept.
 * A sharded engine created with DINT_FLAG_SHARD_REPLICA takes the piece dint_records_route made for it: one check pass reads all n
 * records before the first chunk, and a record that is home to another shard or names a table the workload has not gives DINT_EINVAL
 * with nothing applied (its READ probe would go unanswered and be misread as "row absent"); this costs one synchronisation. */
int dint_log_apply_device(dint_engine_t *e, const void *d_records, uint64_t n, uint32_t chunk, dint_apply_stats *out);

#define DINT_FOLD_DRY_RUN 1u
typedef struct dint_fold_stats {
  uint64_t applied, commits, inserts, deletes, chunks; /* as dint_apply_stats: what the records would have been as backup operations */
  uint64_t rows;             /* distinct (table, key) per chunk, summed over the chunks */
  uint64_t folded_records;   /* records whose row's net effect went to the repair */
  uint64_t deferred_records; /* records that went through the serial replay (dint_log_apply_device's chunk routine) */
  uint64_t deferred_buckets; /* buckets that made them do so, per chunk, summed */
  uint64_t repair_records, updated, inserted, deleted, refused; /* what reached the repair kernel and what it did (dint_repair_stats) */
  uint64_t ns[4];  /* with dint_timing_enable: nanoseconds of [0] the key pass and the sorts, [1] probe, fold and emit, [2] the repair,
                      [3] the deferred records' serial replay */
  uint64_t reserved[5];
} dint_fold_stats;
/* (v5, additive) dint_log_apply_device with every chunk FOLDED first: the records of a chunk are sorted by (table, bucket, key, log
 * index), the replica's chain is probed once per row, and each row's records collapse to their net effect -- the last value and the
 * version the count of commits gives, or "gone" -- which dint_state_repair's kernel writes with one lane per bucket; no hot-path pass
 * sees those records.  The rule is dint_amd/csrc/log_fold.h.  Afterwards every table holds the multiset of rows (key, version, value)
 * that dint_log_apply_device leaves on the same replica, records and chunk, so dint_state_digest is equal; chain layout, holes and
 * pool use may differ ("state is rows only", below).  A bucket in which a row the chunk touches is held twice or more is DEFERRED:
 * all its records of the chunk go through dint_log_apply_device's own chunk routine in log order (folded and deferred buckets are
 * disjoint, so the two write paths commute).
 * Contract, refusals and stream ordering are dint_log_apply_device's (DINT_FLAG_SHARD_REPLICA included: the fold places a row at its
 * local bucket, the whole list is checked before the first chunk, also for a dry run): lock / log / store engines DINT_ESTATE, a sharded engine
 * without that flag DINT_EINVAL, an announced batch pending DINT_ESTATE, d_records == NULL with n > 0 DINT_EINVAL, n == 0 returns 0; flags other than
 * DINT_FOLD_DRY_RUN and records not 16-byte aligned: DINT_EINVAL.  Keys stay below 2^60, as for the serial replay.  The records
 * stay untouched; the replica's lock words, log ring and log cursor are left alone.  FOLDED records are not counted in the
 * replica's request counters (dint_stats batches / requests; nor in missing_keys, which the serial replay bumps for a smallbank
 * record of an absent row): only the deferred ones pass the hot path.  The call is synchronous: per chunk the host waits ONCE,
 * to learn the deferred and repair record counts, and once more at the end of the call; it returns with `out` (may be NULL)
 * filled.  DINT_FOLD_DRY_RUN fills every field except updated / inserted / deleted / refused and
 * writes no table byte (a blank engine stays blank).
 * Pool: the serial replay may need overflow entries only for a while; the fold never needs more than it: in front of every repair launch the
 * pool's pend lists are rotated into its free lists, as a hot-path pass does, so entries a folded delete emptied are allocated
 * again by later chunks and calls although no pass runs.  When an insert of the
 * repair finds the pool full, equality with the unfolded path is not promised; it is reported as dint_state_repair reports it --
 * `refused`, dint_stats.pool_exhausted, DINT_ENOMEM, the rest applied.  Scratch of ~250 bytes per record of a chunk is allocated on
 * the first call and kept, beside dint_log_apply_device's own for the deferred records. */
int dint_log_apply_folded_device(dint_engine_t *e, const void *d_records, uint64_t n, uint32_t chunk, uint32_t flags,
                                 dint_fold_stats *out);
/* ---- state sync (v5, additive): is a replica equal to its primary, what differs, and the repair -- on the device ----------
 * "State" is ROWS ONLY: per table the multiset of valid (key, ver, val) slots.  Lock words, the log ring, the pool's free
 * lists and the chain layout are per server and transient; a replica rebuilt from a log has other chains than its primary.
 * The three calls are for store, tatp and smallbank engines (lock / log engines: DINT_ESTATE), are synchronous like
 * dint_log_drain (they return with their result on the host), order themselves behind the engine's pending work on `stream`
 * (a hipStream_t, NULL = the engine's own) and refuse an engine with a batch announced by dint_submit_device_ahead still
 * pending (DINT_ESTATE, as dint_snapshot).  The caller keeps the engines quiet for the duration. */
typedef struct dint_table_digest {
  uint64_t rows;     /* valid rows of the table (duplicate keys count once per row) */
  uint64_t sum, xr;  /* sum mod 2^64 and xor of the row hashes: fasthash64(bytes, len, 0xdeadbeef) over
                        key (8, LE) | ver (4, LE) | table (1) | 0 0 0 | val (40 or 8) */
  uint64_t reserved;
} dint_table_digest;
/* (v5, additive) out[t] for every table t of the workload (1 / 5 / 2); returns that number (cap_tables smaller: DINT_EINVAL).
 * Commutative on purpose: the digest depends on neither chain layout nor bucket order.  A sharded engine is accepted: the digest
 * is of its local rows (rows and sum add up, xr xors, over the shards).  64 bytes per table reach the host. */
int dint_state_digest(dint_engine_t *e, dint_table_digest *out, uint32_t cap_tables, void *stream);

typedef struct dint_diff_stats {
  uint64_t total;       /* records the full diff has (also when cap is smaller) = only_a + only_b + val_differs + ver_only */
  uint64_t only_a;      /* rows of a that b lacks */
  uint64_t only_b;      /* rows of b that a lacks */
  uint64_t val_differs; /* rows of both whose values differ (whatever the versions) */
  uint64_t ver_only;    /* rows of both that differ in the version alone */
  uint64_t reserved[3];
} dint_diff_stats;
/* (v5, additive) what must be done to b to make its rows equal a's, as canonical 64-byte log records (dint_read_log) in
 * DEVICE memory (8-byte aligned): a row of a that b lacks or holds differently -> {key, a's val zero-padded to 40, a's ver,
 * is_del = 0, table}; a row only b has -> {key, is_del = 1, table}, val and ver zero; pad zero.  Compared are the VISIBLE rows:
 * per key the first valid slot in chain order, what a READ returns (a shadowed duplicate is outside the diff; the digest is the
 * strict check).  The order is fixed: ascending table, ascending bucket; inside a bucket a's rows in a's chain order, then the
 * b-only rows in b's.  Returns the number of records written (<= cap; the first cap of that order); out (may be NULL) says how
 * many there are.  d_records == NULL with cap == 0 only counts.  Neither engine is modified.  Refused before any GPU work:
 * a == b, a null engine, engines of different workloads, table sizes or devices, a sharded engine on either side (DINT_EINVAL)
 * -- unless both engines are the SAME shard (shard_index and shard_count equal) and every sharded one was created with
 * DINT_FLAG_SHARD_REPLICA: then the order is ascending table, ascending LOCAL bucket, what that shard's dint_state_repair takes;
 * lock / log engines, an announced batch pending on either (DINT_ESTATE).  Scratch of 12 bytes per 256 buckets is allocated in
 * a on the first call and kept. */
int64_t dint_state_diff(dint_engine_t *a, dint_engine_t *b, void *d_records, uint64_t cap, dint_diff_stats *out, void *stream);

typedef struct dint_repair_stats {
  uint64_t applied;  /* = updated + inserted + deleted */
  uint64_t updated;  /* the visible row took the record's value and version in place */
  uint64_t inserted; /* the key was absent: kvs_insert placement, the record's version */
  uint64_t deleted;  /* kvs_delete of the visible row (a delete of an absent key changes nothing and is counted nowhere) */
  uint64_t refused;  /* inserts that found the overflow-entry pool full */
  uint64_t reserved[3];
} dint_repair_stats;
/* (v5, additive) applies n records of dint_state_diff's form and ORDER (grouped by bucket: table and bucket ascending) to b WITH THE
 * VERSIONS THEY CARRY -- a resync, not a log replay (dint_log_apply_device bumps versions as the backup operations do).  The
 * records of one bucket are applied in order by one lane; buckets run in parallel.  Records out of order, or naming a table the
 * workload has not: DINT_EINVAL with the tables untouched.  b's lock words, log ring, log cursor and request counters are left
 * alone.  An insert that finds the pool full is not done: `refused` and dint_stats.pool_exhausted count it, the rest is applied,
 * the call returns DINT_ENOMEM (as dint_wait).  Same refusals as dint_state_diff for the one engine.  A sharded engine created with
 * DINT_FLAG_SHARD_REPLICA is taken: "bucket" is then the shard's local bucket (global bucket / shard_count), and a record that is
 * home to another shard is refused like a record out of order -- DINT_EINVAL, tables untouched.  A list in the unsharded order that
 * went through dint_records_route arrives in this order. */
int dint_state_repair(dint_engine_t *b, const void *d_records, uint64_t n, dint_repair_stats *out, void *stream);

/* (v5, additive) ROUTE: the n canonical 64-byte records at d_records (DEVICE memory) partitioned, stably, by their home among
 * dst_count shards -- home = (fasthash64(key) % the table's bucket count) % dst_count, dint_amd/csrc/state_route.h -- into d_out (DEVICE
 * memory on the same device, room for cap records): shard 0's records in their input order, then shard 1's ...; offsets (HOST, dst_count
 * + 1 entries) says where: shard h's records are d_out[offsets[h] .. offsets[h + 1]), offsets[dst_count] = n.  Returns n.  What it
 * is for: a list produced under one layout -- a drained log, a dint_state_diff or dint_state_block_rows list of an unsharded primary or
 * of one shard of G -- becomes the lists of the shards of another; log order per row and the repair's bucket order both survive it.
 * `geom` is any store / tatp / smallbank engine on the device that holds the records (lock / log engines: DINT_ESTATE): only its
 * workload and n_rows, which fix the bucket counts, are used; its own shard layout is ignored, its tables are neither read nor
 * written, and it need not be quiet.  The call orders itself behind the engine's pending work on `stream` (NULL = the engine's own)
 * and synchronises it ONCE, to read the check's result and the offsets; the records are written behind that, in stream order.
 * dst_count == 1 is a copy.  d_records == NULL with n == 0: returns 0, every offset 0.  Refused before a byte of d_out is written:
 * dst_count 0 or above 255, a buffer that is not 16-byte aligned, input and output ranges that overlap, more than 2^32 - 16
 * (shard, 512-record tile) pairs (DINT_EINVAL); cap < n (DINT_ENOMEM); a record whose table the workload has not -- it has no home --
 * (DINT_EINVAL; dint_last_error names the first such index).  Two calls on the same input write the same bytes.  Scratch of 12 bytes
 * per (shard, tile) is allocated in geom on first use, grown to what a call needs and kept. */
int64_t dint_records_route(dint_engine_t *geom, uint32_t dst_count, const void *d_records, uint64_t n, void *d_out, uint64_t cap,
                           uint64_t *offsets, void *stream);

/* ---- block sync (v5, additive): two replicas on DIFFERENT devices compared block by block, only the blocks that differ shipped ----
 * dint_state_diff wants both engines on one device; between two GPUs dint_state_digest says "not equal" and nothing about where,
 * and an image carries everything.  These four calls are the steps in between; what crosses between the devices -- digests one way,
 * block ids back, rows forth -- is plain bytes in device memory that the CALLER moves.
 *
 * A BLOCK is block_buckets consecutive LOCAL buckets of one table (dint_amd/csrc/state_block.h is the rule): block_buckets a power
 * of two, 64 .. 2^20, anything else DINT_EINVAL; a table's last block may be short.  Block ids are u32 and run over the tables in
 * table order: table 0's blocks, then table 1's ...  Two engines of the same workload, n_rows, shard_index / shard_count,
 * DINT_FLAG_LOCK_SAME_KEY and block_buckets have the same blocks, and that is what the caller must pair.  A sharded engine is
 * accepted: it is compared with the same shard of the other set.
 *
 * The contract is the state sync's: synchronous, ordered behind the engine's pending work on `stream` (NULL = the engine's own);
 * store / tatp / smallbank engines only (lock / log engines: DINT_ESTATE); an announced batch pending: DINT_ESTATE; no engine is
 * modified; nothing of a caller's buffer is trusted.  Device buffers are 8-byte aligned (ids: 4).  Scratch is allocated in the
 * engine on first use, grown to what a call needs and kept.  One host synchronisation per call, two for block_rows / block_diff
 * when there is something to write (the total is read first, as dint_state_diff does). */
typedef struct dint_block_digest {
  uint64_t rows, sum, xr; /* as dint_table_digest, over the valid slots of the chains of the block's buckets */
  uint64_t reserved;      /* 0 */
} dint_block_digest;
typedef struct dint_block_stats {
  uint64_t total;         /* block_digest: the blocks; block_rows: the records the listed blocks hold (also when cap is smaller) */
  uint32_t n_blocks;      /* blocks of the engine at this block_buckets */
  uint32_t n_tables;
  uint32_t blocks[5];     /* blocks per table: table t's ids are [blocks[0] + .. + blocks[t - 1], ... + blocks[t]) */
  uint32_t block_buckets;
  uint64_t reserved[3];
} dint_block_stats;
/* (v5, additive) d_out[id] (DEVICE memory, room for cap_blocks digests) = the digest of block id, for every block; returns the number
 * of blocks (cap_blocks smaller: DINT_EINVAL, nothing written).  d_out == NULL only counts.  Digested is every valid slot reached by
 * walking the chains of the block's buckets (bounded by 4096 entries, links checked), shadowed duplicates included: on tables that
 * dint_state_verify finds sound, the blocks of a table merge (rows and sum add, xr xors) to dint_state_digest's entry. */
int64_t dint_state_block_digest(dint_engine_t *e, uint64_t block_buckets, void *d_out, uint64_t cap_blocks, dint_block_stats *out_stats,
                                void *stream);
/* (v5, additive) needs no engine: d_a, d_b = two arrays of n_blocks digests on one device; d_ids (u32, room for cap) takes the
 * ascending ids of the blocks whose 32 bytes differ.  Returns how many there are in all; the first cap are written.  Synchronises
 * `stream` (NULL: the null stream) once; one word of scratch is allocated and freed by the call. */
int64_t dint_state_block_select(const void *d_a, const void *d_b, uint32_t n_blocks, void *d_ids, uint64_t cap, void *stream);
/* (v5, additive) the VISIBLE rows (per key the first valid slot in chain order, as in dint_state_diff) of the n_ids blocks listed in
 * d_ids (DEVICE memory, u32, strictly ascending) as canonical 64-byte records {key, val zero-padded to 40, ver, is_del = 0, table}
 * into d_records.  Order: ascending id, ascending bucket, chain order.  Returns the records written (the first cap of that order);
 * out_stats->total how many there are.  d_records == NULL with cap == 0 only counts.  Ids not strictly ascending or out of
 * range: DINT_EINVAL, nothing written. */
int64_t dint_state_block_rows(dint_engine_t *e, uint64_t block_buckets, const void *d_ids, uint32_t n_ids, void *d_records, uint64_t cap,
                              dint_block_stats *out_stats, void *stream);
/* (v5, additive) what must be done to b INSIDE the listed blocks to make its visible rows those of the row list d_rows (n_rows
 * records of dint_state_block_rows' form and order, DEVICE memory on b's device), in dint_state_diff's record form, order and
 * stats: ascending table and bucket; the list's rows of a bucket in list order, then b's rows that the list lacks in b's chain
 * order.  The output goes to dint_state_repair unchanged.  A check reads the whole list before anything is written: every row's
 * table is in range and it is no delete record, every row is home (fasthash64 % hash size, shard included) to a bucket of a
 * listed block, (table, bucket) is non-decreasing, no bucket has more than 16,384 rows; ids as for block_rows.  A list or id
 * list that fails: DINT_EINVAL with not a byte written.  A key that appears twice in one bucket's run: the first is the visible
 * one.  n_rows >= 2^32 - 16: DINT_EINVAL. */
int64_t dint_state_block_diff(dint_engine_t *b, uint64_t block_buckets, const void *d_ids, uint32_t n_ids, const void *d_rows, uint64_t n_rows,
                              void *d_records, uint64_t cap, dint_diff_stats *out_stats, void *stream);

/* ---- state image (v5, additive): an engine's tables moved to another shard layout, cloned or checkpointed -- on the device ----
 * An IMAGE holds everything of one source engine that belongs to one destination shard, entry for entry: kv workloads -- the
 * inline entries (whole stride: keys, versions, valid bytes, values, tatp lock bytes, smallbank counters, owner keys) and every
 * bucket's overflow entries in chain order, links made image-relative, invalid slots and shadowed duplicates where they were;
 * lock tables -- the slots.  Not in it: the log ring, the pool's free and pend lists, pass scratch.  The byte layout is in
 * dint_amd/csrc/state_image.h.  An image is plain bytes: any copy carries it to another GPU or a file.  Both calls are
 * synchronous like dint_state_diff, order themselves behind the engine's pending work on `stream` (NULL = the engine's own) and
 * refuse a log_server engine and an engine with a batch announced by dint_submit_device_ahead still pending (DINT_ESTATE).
 * The caller keeps the engine quiet for the duration. */
typedef struct dint_image_stats {
  uint64_t bytes;             /* size of the image */
  uint64_t buckets;           /* kv: buckets; lock tables: slots */
  uint64_t overflow_entries;  /* chain entries beyond the inline ones */
  uint64_t rows;              /* valid slots (lock tables: slots with a non-zero word) */
  uint64_t reserved[4];
} dint_image_stats;
/* (v5, additive) the image of every global bucket / slot g that src owns with g % dst_count == dst_index (dst_count 0 or 1:
 * unsharded) into d_buf (device memory, 16-byte aligned).  src may itself be sharded (i, G): the piece for (j, H) is non-empty
 * only if i == j mod gcd(G, H); an empty piece is a valid image of zero buckets.  d_buf == NULL or cap_bytes == 0 counts only
 * and fills out->bytes; a buffer that is too small: DINT_ENOMEM with out->bytes set and nothing written.  src is left untouched. */
int dint_state_export(dint_engine_t *src, uint32_t dst_index, uint32_t dst_count, void *d_buf, uint64_t cap_bytes, dint_image_stats *out,
                      void *stream);
/* (v5, additive) the image's buckets to g / dst_count of dst; its overflow entries become one contiguous range of each table's
 * pool (one bump of pool_top; free lists are not consulted).  dst must be BLANK: created or dint_reset, and since then nothing
 * but imports (DINT_ESTATE otherwise); a piece is (source index, source count), importing one twice is DINT_ESTATE.  Refused
 * before any table byte changes: an image of another workload, flags (DINT_FLAG_LOCK_SAME_KEY), n_rows / n_slots, or addressed
 * to another (index, count) than dst's (DINT_EINVAL); fewer free pool entries than it needs (DINT_ENOMEM); a malformed image
 * (DINT_EINVAL: nothing of an image is trusted, a check kernel reads all of it before a table is touched -- sizes against
 * `bytes`, ids ascending, in range and home to dst, every link 0, 1 or inside its bucket's run of overflow entries, the chain
 * visiting that run exactly once and in order).  dst's log ring, drain cursor and dint_stats stay as they were. */
int dint_state_import(dint_engine_t *dst, const void *d_buf, uint64_t bytes, dint_image_stats *out, void *stream);

/* ---- rehash (v5, additive): the rows of a set of engines placed into a blank engine of another n_rows -- on the device ----
 * An image moves buckets whole and so cannot change the bucket counts fixed at dint_engine_create.  A rehash moves ROWS: dst
 * (store, tatp or smallbank; its own n_rows, shard_index / shard_count and pool_entries) takes every row of srcs[0 .. n_srcs)
 * whose key is home to it under its own geometry -- g' = fasthash64(key) % dst's hash size of the table, g' % shard_count ==
 * shard_index, local bucket g' / shard_count.  The sources may be any set, sharded or not; whether they are a complete shard
 * set is the caller's business.  The layout is fixed (dint_amd/csrc/state_rehash.h): the rows that land in a bucket, taken in
 * SOURCE ORDER -- position of the engine in srcs, local bucket, chain order, slot: dint_dump_rows order, engine after engine,
 * shadowed duplicates included -- fill the bucket's inline entry (chain position 0, head = 1) and then overflow entries without
 * holes; the overflow entries of all buckets are one contiguous range of the pool in bucket order (one bump of pool_top per
 * table, free lists not consulted).  Key, version and value are copied verbatim, so every key's visible row stays its visible
 * row and dint_state_digest adds up.  Lock words cannot move (a lock word belongs to hash % (4 hash_size), not to a key): dst's
 * lock bytes, counters and owner keys are zero, and sources that hold any are refused unless DINT_REHASH_DROP_LOCKS is set.
 * Synchronous like dint_state_import; orders itself behind every engine's pending work on `stream` (NULL = dst's own); the
 * caller keeps all engines quiet for the duration.  The sources are only read; dst's log ring, drain cursor and dint_stats
 * stay as they were.  Every refusal comes before any table byte of dst changes, and dst stays blank:
 *   DINT_EINVAL  n_srcs == 0 or > 255, dst among srcs, a source twice, engines of different workloads, DINT_FLAG_LOCK_SAME_KEY
 *                settings or devices, a table of more than 2^32 - 16 rows
 *   DINT_ESTATE  a lock_fasst / lock_2pl / log engine (no keys; n_slots cannot be changed this way); dst not blank (created or
 *                dint_reset and nothing since -- an engine that has imported pieces holds rows and is refused too); a batch
 *                announced by dint_submit_device_ahead pending on any engine; a source chain that does not end within 4096
 *                entries or leaves the pool; lock words held without DINT_REHASH_DROP_LOCKS (out->locks_held says how many); a
 *                destination bucket that would need more than 4095 overflow entries
 *   DINT_ENOMEM  a table needs more overflow entries than dst's pool has: out->table[t].overflow_entries is the need, so the
 *                caller can create a destination that fits (dint_config.pool_entries)
 * `out` (may be NULL) is filled as far as the call got, also when it refuses.  After a successful call dst is no longer blank. */
#define DINT_REHASH_DROP_LOCKS 1u
typedef struct dint_rehash_stats {
  uint64_t rows_seen;    /* valid slots of the sources */
  uint64_t rows_placed;  /* ... of them home to dst */
  uint64_t rows_foreign; /* ... and home to another shard of dst's layout */
  uint64_t locks_held;   /* non-zero tatp lock bytes / smallbank counter pairs of the sources (dropped, or the reason of the refusal) */
  struct {
    uint64_t rows;             /* rows placed in the table */
    uint64_t overflow_entries; /* overflow entries they need (pool_top afterwards) */
    uint64_t longest_chain;    /* entries of the longest chain, the inline entry included */
    uint64_t reserved;
  } table[5];
  uint64_t stage_ns[5]; /* with dint_timing_enable(dst, 1): nanoseconds of count, keys, sort, plan, build between events */
  uint64_t reserved[3];
} dint_rehash_stats;
int dint_state_rehash(dint_engine_t *dst, dint_engine_t *const *srcs, uint32_t n_srcs, uint32_t flags, dint_rehash_stats *out,
                      void *stream);

/* ---- bulk load (v5, additive): rows loaded and the population generated -- on the device ---------------------------------
 * dint_load_rows_device is dint_load_rows for DEVICE arrays: keys[n] (8-byte aligned), vers[n] (4-byte aligned; NULL: version
 * 0), vals[n][val_size] (8-byte aligned), n < 2^32 - 16, rows in insertion order.  The tables afterwards are what n kvs_insert
 * calls in that order leave (dint_amd/csrc/state_load.h is the rule): rows home to another shard are skipped and counted,
 * duplicate keys are rows like any other, chains run newest entry first.
 *   A table that has taken nothing since dint_engine_create / dint_reset is built DIRECTLY: hash, stable sort by local bucket,
 *   scan of the overflow entries, one host synchronisation to compare the need with the pool, then every entry written whole
 *   by one lane group.  Overflow entries are pool 0 .. need - 1 in (bucket, insertion) order, pool_top takes one store, lock
 *   bytes / owner keys / smallbank counters are not written.  Refused with nothing written: DINT_ENOMEM when the table needs
 *   more overflow entries than the pool has (out->table[t].overflow_entries is the need, as dint_state_rehash reports it);
 *   DINT_ESTATE when a bucket would need more than 4095 overflow entries.  The table stops being untouched, the engine blank.
 *   Any other table takes the rows as load-mode passes formed on the device from the arrays: result and refusals are
 *   dint_load_rows's (out->direct = 0; overflow_entries and longest_chain_entries are not known then and stay 0).
 * DINT_EINVAL: a null or misaligned array, a bad table, n too large.  DINT_ESTATE: a workload without kv tables, a batch announced
 * by dint_submit_device_ahead pending.  Synchronous; runs on `stream` (NULL = the engine's own) behind the engine's pending work.
 *
 * dint_populate_device is dint_populate without the host: table by table the reference's rows for the first populate_n
 * subscribers / accounts are generated on the device in insertion order and loaded directly.  The engine must be blank
 * (DINT_ESTATE otherwise); a sharded engine generates everything and keeps its home rows.  Temporary device memory is one
 * table's rows and plan at a time, freed before the call returns; out->temp_bytes is the peak.  A refusal of a table's load
 * leaves that table and the ones behind it empty, the ones before it loaded. */
typedef struct dint_load_stats {
  uint64_t rows_loaded;  /* rows home to this engine */
  uint64_t foreign_rows; /* rows home to another shard (skipped) */
  struct {
    uint64_t rows;                  /* home rows of the table */
    uint64_t overflow_entries;      /* the table's need (direct loads; also when refused) */
    uint64_t longest_chain_entries; /* entries of its longest chain, the inline entry included (direct loads) */
    uint64_t direct;                /* 1: built directly, 0: loaded by passes (or not loaded by this call) */
  } table[5];
  uint64_t direct;      /* 1: every table this call loaded was built directly */
  uint64_t temp_bytes;  /* peak temporary device memory of the call */
  uint64_t stage_ns[6]; /* with dint_timing_enable: generate, keys, sort, plan, build between events, summed over the tables; [5] the
                           host pre-pass of the data-dependent tatp tables (0 when the process had it cached) */
  uint64_t reserved[4];
} dint_load_stats;
int dint_load_rows_device(dint_engine_t *e, uint32_t table, const uint64_t *d_keys, const uint32_t *d_vers, const void *d_vals, uint64_t n,
                          dint_load_stats *out, void *stream);
int dint_populate_device(dint_engine_t *e, uint64_t populate_n, dint_load_stats *out, void *stream);
/* ---- table report (v5, additive): occupancy and chain shape of an engine's tables -- read where they lie ----------------
 * What tells an operator WHEN to rehash: how full the buckets are, how long the chains, how much of the overflow pool is
 * linked, how many slots are holes or shadowed duplicates, whether lock words are held (dint_state_rehash refuses those).
 * Every bucket's chain is walked once on the device (dint_amd/csrc/state_stats.h is the rule; header sectors only, values
 * are never read); about 640 bytes per table reach the host.  Exact, and independent of scheduling. */
typedef struct dint_table_stats {
  uint64_t buckets;            /* local buckets */
  uint64_t buckets_empty;      /* ... without a valid slot */
  uint64_t rows;               /* valid slots reached by the walk (= dint_table_digest.rows while no valid slot sits outside a chain) */
  uint64_t entries;            /* entries linked into chains, the inline entry included when it is linked */
  uint64_t overflow_entries;   /* the pool entries among them */
  uint64_t holes;              /* 4 * entries - rows */
  uint64_t inline_first;       /* buckets whose chain starts with the inline entry */
  uint64_t inline_unlinked;    /* buckets with a non-empty chain that does not contain the inline entry */
  uint64_t hit_entries;        /* over all valid slots: position of the slot's entry in its chain + 1; / rows = header sectors per lookup of a stored row */
  uint64_t shadowed_rows;      /* valid slots whose key an earlier valid slot of the bucket holds (chain order): rows - distinct keys */
  uint64_t buckets_unchecked;  /* buckets of more than 64 entries: walked and counted, but their keys are not compared (nothing in shadowed_rows) */
  uint64_t longest_chain;      /* entries of the longest chain */
  uint64_t longest_chain_bucket; /* the lowest global bucket id (local * shard_count + shard_index) that attains it; UINT64_MAX: a table without rows */
  uint64_t most_rows;          /* valid slots of the fullest bucket */
  uint64_t locks_held;         /* non-zero tatp lock bytes / smallbank {num_ex, num_sh} pairs with a non-zero word (as dint_rehash_stats.locks_held); store: 0 */
  uint64_t pool_cap, pool_top; /* the overflow pool: entries it has / handed out so far (pool_top - overflow_entries: reusable or leaked) */
  uint64_t chain_hist[17];     /* buckets by entries in the chain: 0 .. 15, [16] = 16 or more */
  uint64_t rows_hist[33];      /* buckets by valid slots: 0 .. 31, [32] = 32 or more */
  uint64_t reserved[13];
} dint_table_stats;
/* (v5, additive) out[t] for every table t of the workload (1 / 5 / 2); returns that number (cap_tables smaller: DINT_EINVAL).
 * Synchronous like dint_state_digest: orders itself behind the engine's pending work on `stream` (NULL = the engine's own),
 * one host synchronisation for all tables.  Read-only: tables, lock words, dint_stats, the log ring and the drain cursor stay
 * as they were, and a blank engine stays blank (it reports zeros and can still be imported or rehashed into).  A sharded engine
 * reports its local buckets.  Refused: a lock_fasst / lock_2pl / log engine (no keys, no chains), a batch announced by
 * dint_submit_device_ahead pending (DINT_ESTATE); a chain that does not end within 4096 entries, visits its inline entry twice
 * or leaves the pool (DINT_ESTATE; dint_last_error names the table).  The caller keeps the engine quiet for the duration. */
int dint_state_stats(dint_engine_t *e, dint_table_stats *out, uint32_t cap_tables, void *stream);
/* ---- table verify (v5, additive): are an engine's tables and overflow pool structurally sound? ---------------------------
 * Every other state call assumes they are.  This one checks, where the tables lie: an exact census of every chain, every free
 * list and every pend list of every table, each pool entry claimed by whatever reaches it first, and the violations counted
 * (dint_amd/csrc/state_verify.h is the rule).  Violations are not an error: they are the report.  While bad_chains,
 * cross_linked and list_bad_links are 0,  linked + free_entries + pending_entries - linked_beyond_top + unaccounted ==
 * min(pool_top, pool_cap);  always stray_rows >= stray_valid_entries. */
#define DINT_VERIFY_RECLAIM 1u /* dint_state_verify flags: put the unaccounted pool entries back on the free lists */
typedef struct dint_table_verify {
  uint64_t pool_cap, pool_top;  /* the overflow pool: entries it has / handed out so far (raw, also above pool_cap) */
  uint64_t rows;                /* valid slots reached by the chain walks */
  uint64_t linked;              /* distinct pool entries linked into chains */
  uint64_t free_entries;        /* ... on the 64 free lists */
  uint64_t pending_entries;     /* ... on the two sets of 64 pend lists */
  uint64_t unaccounted;         /* ... below pool_top that no chain and no list reaches: leaked */
  uint64_t longest_list;        /* entries of the longest free or pend list */
  uint64_t bad_chains;          /* chains that do not end within 4096 entries, visit their inline entry twice or leave the pool */
  uint64_t cross_linked;        /* times a chain or list met an entry another chain or list (or that list itself) holds */
  uint64_t linked_beyond_top;   /* pool entries at or above pool_top that a chain or a list reaches */
  uint64_t list_bad_links;      /* lists that end in a link of 1 or beyond the pool */
  uint64_t stray_valid_entries; /* entries outside every chain with a valid byte set (a flat scan counts their slots) */
  uint64_t stray_rows;          /* ... the valid slots they hold */
  uint64_t misplaced_rows;      /* valid slots whose key hashes to another bucket or shard: no request finds them */
  uint64_t odd_valid_bytes;     /* valid bytes that are neither 0 nor 1 */
  uint64_t reclaimed;           /* DINT_VERIFY_RECLAIM: the unaccounted entries put back on the free lists */
  uint64_t stray_rows_cleared;  /* ... and the valid slots their headers held */
  uint64_t reserved[14];        /* out[0].reserved[11..13], with dint_timing_enable: nanoseconds of the chain stage, the list stage, the pool stage
                                   and sum, all tables, between events */
} dint_table_verify;
/* (v5, additive) out[t] for every table t of the workload (1 / 5 / 2); returns that number (cap_tables smaller: DINT_EINVAL).
 * Synchronous like dint_state_stats: orders itself behind the engine's pending work on `stream` (NULL = the engine's own), one
 * host synchronisation for all tables.  flags = 0: read-only -- nothing of the engine changes and a blank engine stays blank.
 * DINT_VERIFY_RECLAIM: when bad_chains, cross_linked, linked_beyond_top and list_bad_links are 0 in every table, each table's
 * unaccounted entries go back to its free lists in ascending order, entry r to list r % 64, their {validw, next} zeroed; the
 * report is the census BEFORE the repair plus `reclaimed`.  With one of those violations in any table not a byte is written
 * and the call returns DINT_ESTATE after filling `out`.  The engine stops being blank only if something was reclaimed.  Refused: a
 * lock_fasst / lock_2pl / log engine, a batch announced by dint_submit_device_ahead pending (DINT_ESTATE).  No content of the
 * tables makes the kernels read or write outside them or loop without bound.  The caller keeps the engine quiet meanwhile. */
int dint_state_verify(dint_engine_t *e, dint_table_verify *out, uint32_t cap_tables, uint32_t flags, void *stream);
/* ---- table compaction (v5, additive): chains packed and the overflow pool made one range, IN PLACE -------------------------
 * What puts right what dint_state_stats diagnoses, without a second engine: at the same bucket count and shard no row changes
 * its bucket, so each bucket's valid rows, in chain order, are packed into its inline entry and as few overflow entries as they
 * need, the overflow entries of all buckets laid end to end from pool entry 0 (dint_amd/csrc/state_compact.h is the rule:
 * dint_state_rehash's layout applied to the engine itself).  pool_top falls to the overflow entries linked; the free and pend
 * lists are emptied (their tags bumped); holes, entries without a valid slot, leaked entries and everything on the lists are
 * dropped.  Chain order is kept, so every key's visible row stays its visible row, and the tatp lock bytes and owner keys and
 * smallbank's counters in the inline entries keep their bytes: an engine that holds locks can be compacted.  The census of
 * dint_state_verify runs first, in the same call. */
#define DINT_COMPACT_DRY_RUN 1u /* dint_state_compact flags: fill the report with what a compaction would do; write nothing */
typedef struct dint_table_compact {
  dint_table_verify verify;     /* the census BEFORE the move (reclaimed = stray_rows_cleared = 0) */
  uint64_t rows;                /* valid rows: every one is kept.  This field and the eleven below are 0 in a refused call */
  uint64_t entries_before, entries_after;   /* entries linked into chains, linked inline entries included */
  uint64_t overflow_before, overflow_after; /* the pool entries among them */
  uint64_t pool_top_before, pool_top_after; /* before: raw, also above pool_cap; after = overflow_after */
  uint64_t holes_before, holes_after;       /* 4 * entries - rows */
  uint64_t buckets_rewritten;   /* buckets whose chain was not yet inline entry first, every entry full but the last */
  uint64_t unaccounted_dropped; /* leaked pool entries that fell below the new pool_top's tail: verify.unaccounted */
  uint64_t staging_bytes;       /* overflow_after * stride: what the table's staging buffer must hold */
  uint64_t reserved[20];        /* out[0].reserved[0..3], with dint_timing_enable: nanoseconds of the census, the count and its scans, the
                                   move, the commit, all tables, between events */
} dint_table_compact;
/* (v5, additive) out[t] for every table t of the workload (1 / 5 / 2); returns that number (cap_tables smaller: DINT_EINVAL).
 * Synchronous like dint_state_verify: orders itself behind the engine's pending work on `stream` (NULL = the engine's own).  The
 * moving kernels read the census on the device, so the call makes one host synchronisation -- two when a table's staging buffer
 * (engine scratch of staging_bytes, allocated by the first call that needs it and kept) has to grow: the kernels do nothing
 * then, and the call runs again with a buffer that fits.  A blank engine stays blank; a second compaction changes nothing but
 * the lists' tags.  Refused, with not a byte written:
 *   DINT_ESTATE  bad_chains, cross_linked, linked_beyond_top, list_bad_links, stray_valid_entries, misplaced_rows or
 *                odd_valid_bytes non-zero in any table (`out` holds the census; unaccounted entries are no violation); a
 *                lock_fasst / lock_2pl / log engine; a batch announced by dint_submit_device_ahead pending
 *   DINT_ENOMEM  a staging buffer cannot be allocated
 *   DINT_EINVAL  an unknown flag, cap_tables too small
 * dint_snapshot captures the tables, pool_next and the control words (pool_top, every head word), so a snapshot taken before a
 * compaction restores the engine as it was before it.  No content of the tables makes the kernels read or write outside them
 * and the staging buffer or loop without bound.  The caller keeps the engine quiet meanwhile. */
int dint_state_compact(dint_engine_t *e, dint_table_compact *out, uint32_t cap_tables, uint32_t flags, void *stream);
/* ---- traffic report (v5, additive): a batch's hot keys, reply codes and shared lock slots -- read where the batch lies ----------
 * The tables have dint_state_stats; this is the same for the REQUEST STREAM: what one batch of wire messages (and, optionally, the
 * replies it got) looks like in the terms DESIGN.md 3 decides a pass's speed by -- requests per key and per unit of serial order,
 * keys that share a unit or a lock slot, REJECT / NOT_EXIST replies.  dint_amd/csrc/traffic_report.h is the rule (decode, class of a
 * request, flags of a reply, unit, lock slot); lock_fasst, lock_2pl, store, tatp and smallbank engines (log_server: DINT_ESTATE).
 * Every number is exact and independent of scheduling.  All sizes are the GLOBAL ones of the engine's configuration: a shard
 * reports what the unsharded engine reports over the same arrays. */
typedef struct dint_traffic_key {
  uint64_t key;          /* the key (lock tables: the lid) */
  uint32_t table;
  uint32_t requests;     /* keyed requests on (table, key): = reads + locks + unlocks + writes + the OTHER class */
  uint32_t reads, locks, unlocks, writes;
  uint32_t rejects, misses; /* replies flagged REJECT / MISS (0 without a reply array) */
  uint32_t first_index;  /* the lowest request index of the key */
  uint32_t reserved;     /* 0 */
} dint_traffic_key;
struct dint_traffic_report { /* (a struct tag only: the call below has the name) */
  uint64_t n;            /* requests of the batch */
  uint64_t keyed;        /* requests with a table the workload has that are no LOG request: what everything per key is over */
  uint64_t bad_table;    /* requests whose table byte names a table the workload has not: counted here and nowhere else */
  uint64_t log_requests; /* tatp COMMIT_LOG / DELETE_LOG, smallbank COMMIT_LOG: in the type histograms and here only */
  uint64_t reads, locks, unlocks, writes, others; /* the keyed requests by class */
  uint64_t rejects, misses;                       /* replies of keyed requests flagged REJECT / MISS */
  uint64_t distinct_keys;       /* distinct (table, key) among the keyed requests */
  uint64_t distinct_units;      /* distinct units: lock tables the lock slot, kv the (table, bucket) */
  uint64_t distinct_lock_slots; /* tatp / smallbank: distinct (table, lock slot) the LOCK / UNLOCK / WRITE-PRIM requests touch; else 0 */
  uint64_t max_key_requests, max_unit_requests;
  uint64_t max_unit, max_unit_table; /* the unit that attains max_unit_requests: the lowest table, then the lowest unit id (n == 0: 0, 0) */
  uint64_t shared_units;         /* units that at least 2 distinct keys of the batch touch */
  uint64_t shared_unit_requests; /* keyed requests on them */
  uint64_t shared_unit_rejects;  /* REJECT replies on them */
  uint64_t shared_slots;         /* tatp / smallbank: lock slots that LOCK / UNLOCK / WRITE-PRIM requests of at least 2 distinct keys touch */
  uint64_t shared_slot_requests; /* ... those requests on them */
  uint64_t shared_slot_rejects;  /* ... their REJECT replies */
  uint64_t n_by_requests, n_by_rejects; /* entries written to the two lists */
  uint64_t temp_bytes;           /* temporary device memory the call allocated and freed; host form: 0 */
  uint64_t reserved[5];
  uint64_t key_hist[25];         /* bin b: distinct keys with 2^b <= requests < 2^(b+1) */
  uint64_t unit_hist[25];        /* ... distinct units */
  uint64_t req_types[5][32];     /* per table: requests by type byte, bin 31 = every byte >= 31 (LOG requests included) */
  uint64_t rep_types[5][32];     /* ... replies by type byte, under the REQUEST's table (all 0 without a reply array) */
};
#define DINT_TRAFFIC_MAX_N (1ull << 24)
#define DINT_TRAFFIC_MAX_TOP 4096u
/* (v5, additive) the report of the n wire messages at d_reqs (DEVICE memory, any alignment) and -- d_replies != NULL -- of the
 * replies they got, replies[i] answering reqs[i] (any alignment; NULL: every reply-derived field is 0 and the by-rejects list
 * empty).  by_requests / by_rejects: HOST arrays of top_k entries (top_k <= 4096; 0: no lists, the pointers may be NULL) that take
 * the keys with the most requests / the most REJECT replies (only keys with at least one), ordered by that count descending, then
 * table ascending, then key ascending -- the order and the cut are deterministic.  Read-only: the call reads the two arrays and the
 * engine's geometry; it writes no table, no pass scratch and no dint_stats, needs no quiet engine, and leaves a batch announced by
 * dint_submit_device_ahead pending.  It runs on `stream` (a hipStream_t, NULL = the engine's own), ordered behind what that
 * stream holds and behind the engine's pending work, and is a diagnostic BESIDE the passes: it synchronises the stream THREE
 * times (the keyed count, the distinct keys, the result) and returns with everything on the host.  Temporary device memory of
 * about 160 bytes per request is the call's own: allocated by the call and freed before it returns (the free waits for the device
 * to be idle); the engine object holds none of it, and nothing of the engine's own memory or of its other calls changes.
 * Refused with nothing written to out or the lists: a null engine / d_reqs with n > 0 / out, lists missing with top_k > 0,
 * top_k > 4096, n > 2^24, d_replies == d_reqs -- an in-place reply has lost the request's type: keep the pristine copy --
 * (DINT_EINVAL); a log_server engine (DINT_ESTATE). */
int dint_traffic_report(dint_engine_t *e, const void *d_reqs, const void *d_replies, uint64_t n, uint32_t top_k,
                        struct dint_traffic_report *out, dint_traffic_key *by_requests, dint_traffic_key *by_rejects, void *stream);
/* ---- held locks (v5, additive): which lock units a server holds, and the release of orphaned ones -- where they lie -----------
 * A coordinator that dies between ACQUIRE and COMMIT / ABORT leaves its locks held for good: no release checks an owner, and from
 * then on every request on the slot is answered REJECT.  dint_state_locks lists the held units from the device, dint_state_unlock
 * releases the listed ones -- or all -- by compare and release (dint_amd/csrc/state_locks.h is the rule).  lock_fasst, lock_2pl, tatp
 * and smallbank engines, sharded or not; store and log_server: DINT_ESTATE.
 *   unit, held iff:  lock_fasst  d_lock_tbl[local slot] = {lock, ver}: lock != 0 (a non-zero version alone is not a held lock)
 *                    lock_2pl    {num_ex, num_sh}: either non-zero
 *                    tatp        byte q of the lock word of local bucket l's inline header: non-zero
 *                    smallbank   pair q of the counters of local bucket l's inline entry: either word non-zero */
#define DINT_LOCK_KEY_OWNER 1u /* dint_lock_record.flags: tatp with DINT_FLAG_LOCK_SAME_KEY -- key is the recorded owner of the unit */
#define DINT_LOCK_KEY_ROW 2u   /* otherwise, cand_rows > 0: key is the first candidate row in chain order */
#define DINT_LOCK_WALK_CUT 4u  /* the chain walk stopped at its bound (4096 entries), at a second visit of the inline entry or at a link
                                  outside the pool (dint_state_block_digest's bound and link check): cand_rows is what was seen up to there */
typedef struct dint_lock_record {
  uint64_t slot;      /* the LOCAL slot index exactly as dint_read_locks numbers it: lock tables global slot / shard_count; kv q * n_local + local bucket */
  uint32_t a, b;      /* as dint_read_locks: {lock, ver}, {num_ex, num_sh}, {lock byte, 0} */
  uint64_t key;       /* see flags; 0 when neither KEY flag is set (always for the lock tables: a lid is not stored) */
  uint32_t cand_rows; /* kv: valid slots in the chain of the unit's bucket whose key's lock slot is this unit, fasthash64(key) % (4 * hash_size)
                         == q * hash_size + global bucket; shadowed duplicates count, holes do not */
  uint8_t table, flags;
  uint16_t zero;
} dint_lock_record;
typedef struct dint_lock_stats {
  uint64_t total;        /* held units in all (also when cap cut the list) */
  uint64_t held[5];      /* ... per table (= dint_table_stats.locks_held) */
  uint64_t sum_a, sum_b; /* over the held units: lock_2pl / smallbank the exclusive and the shared holders */
  uint64_t no_row;       /* kv units with cand_rows == 0 */
  uint64_t walk_cut;     /* kv units with DINT_LOCK_WALK_CUT */
  uint64_t reserved[6];
} dint_lock_stats;
/* (v5, additive) the held units as 32-byte records into d_records (DEVICE memory, 8-byte aligned, room for cap records), in the order
 * ascending table, then ascending local bucket, then ascending q (lock tables: ascending local slot); returns the records written
 * = the first `cap` of that order, out->total says how many there are.  d_records == NULL with cap == 0 only counts.  Positions come
 * from a count per workgroup, a scan and wave ballots -- no atomic decides one, two calls write the same bytes.  Synchronous like
 * dint_state_stats: ordered behind the engine's pending work on `stream` (NULL = the engine's own), one host synchronisation.
 * Read-only: tables, lock words, dint_stats, the log ring and its cursor stay as they were, a blank engine stays blank and a fresh
 * table fresh.  Refused: a store / log_server engine, a batch announced by dint_submit_device_ahead pending (DINT_ESTATE); a
 * misaligned buffer, d_records == NULL with cap > 0 (DINT_EINVAL).  No content of the tables makes the kernels read outside them or
 * write outside the cap records.  The caller keeps the engine quiet meanwhile. */
int64_t dint_state_locks(dint_engine_t *e, void *d_records, uint64_t cap, dint_lock_stats *out, void *stream);
#define DINT_UNLOCK_ALL 1u     /* dint_state_unlock flags: every held unit (d_records == NULL, n == 0) */
#define DINT_UNLOCK_DRY_RUN 2u /* the same check, counts and return value; nothing is written */
typedef struct dint_unlock_stats {
  uint64_t released;               /* units set free (dry run: that would be) */
  uint64_t stale;                  /* list form: units left alone because they no longer hold what their record says */
  uint64_t released_a, released_b; /* the counter sums given up (lock_fasst: a only) */
  uint64_t per_table[5];           /* released, per table */
  uint64_t reserved[7];
} dint_unlock_stats;
/* (v5, additive) LIST FORM: n records of dint_state_locks' form and order in DEVICE memory (8-byte aligned) -- its output or any
 * sub-sequence of it.  The whole list is read before a byte is written and refused with DINT_EINVAL, tables untouched and
 * dint_last_error naming the first such index, for: a table the workload has not; a slot outside the engine's local range, or on a
 * sharded kv engine a unit whose global bucket lies beyond the table; records not strictly ascending in (table, bucket, q); a record
 * with a == 0 && b == 0 (lock_fasst: a == 0).  Then COMPARE AND RELEASE, one lane per record: a unit is released only if its
 * current {a, b} equals the record's (lock_fasst: a alone, the version moves independently) and, for a record with
 * DINT_LOCK_KEY_OWNER on a DINT_FLAG_LOCK_SAME_KEY engine, the stored owner key equals the record's key; otherwise it is left alone
 * and counted `stale` (released and taken again since the listing, or free by now).  key without KEY_OWNER, cand_rows and the other
 * flags of an input record are ignored.  DINT_UNLOCK_ALL: a sweep over the listing's ranges releases every held unit.  A release
 * writes what the workload's own release leaves: lock_fasst lock = 0, version untouched; lock_2pl / smallbank both counters 0; tatp
 * the one lock byte 0 by a byte store, the owner key left as an ABORT leaves it.  Never written: rows, versions, valid bytes,
 * links, the pool, the log ring and its cursor, dint_stats, the blank and the freshness gates.  Synchronous, ordered as
 * dint_state_locks, one host synchronisation (the releasing kernel reads the check's verdict on the device).  Returns 0.  Refused
 * besides: unknown flags, DINT_UNLOCK_ALL with a list, a NULL list with n > 0, a misaligned buffer, n >= 2^32 - 16 (DINT_EINVAL); a
 * store / log_server engine, an announced batch pending (DINT_ESTATE).  The caller keeps the engine quiet meanwhile. */
int dint_state_unlock(dint_engine_t *e, const void *d_records, uint64_t n, uint32_t flags, dint_unlock_stats *out, void *stream);
int dint_get_stats(dint_engine_t *e, dint_stats *out);
/* reset tables, locks, log and stats to the freshly-created (unpopulated) state */
int dint_reset(dint_engine_t *e);
/* snapshot / restore the whole engine state in HBM (used to replay a recorded trace) */
int dint_snapshot(dint_engine_t *e);
int dint_restore(dint_engine_t *e);

/* ---- multi-GPU routing -------------------------------------- */
/* One step on rank r of G (every engine created with shard_index = r, shard_count = G):
 *   dint_route_pack      stable partition of the ingested batch by home rank into G fixed-capacity slots
 *   all-to-all           of the slots (RCCL; equal split sizes, so no host round trip)
 *   dint_submit_segments the home engine answers what it received, in (source rank, index) order, in place
 *   all-to-all           back
 *   dint_route_unpack    replies to their original positions
 * A slot = seg_cap messages at d_send + w * seg_stride, with its live count (u32) at d_cnt + w * cnt_stride (the
 * caller decides where the header lives, e.g. in front of the slot so that it travels with it).  d_slot[n] (u32)
 * remembers where each request went.  Requests beyond a slot's capacity are not sent: dint_route_unpack answers them
 * with the back-pressure reply of dint_refuse, which every client answers by sending the request again
 * (dint_stats.route_overflow counts them); n <= 1,048,576 and G <= 64 per call. */
int dint_route_pack(dint_engine_t *e, const void *d_reqs, uint32_t n, void *d_send, uint32_t seg_cap,
                    uint64_t seg_stride, void *d_cnt, uint64_t cnt_stride, uint32_t *d_slot, void *stream);
int dint_route_unpack(dint_engine_t *e, const void *d_back, uint32_t seg_cap, uint64_t seg_stride,
                      const uint32_t *d_slot, const void *d_reqs, uint32_t n, void *d_replies, void *stream);
/* The same for several batches at once -- the S logical servers of a rank (3 for tatp / smallbank), each routed with
 * its own engine's hash and modulus -- in ONE set of kernel launches (grid.y = batch): a step then costs 3 + 1 launches
 * on the exchange stream whatever S is.  d_slots = this batch's slot of peer 0 (peer w at + w * seg_stride) in the send
 * buffer (pack) or in the returned buffer (unpack); d_cnt = its live-count word of peer 0 (peer w at + w *
 * cnt_stride).  At most 4 batches per call, all on one device; callers pass the engines in the same order. */
typedef struct dint_route_item {
  dint_engine_t *engine;
  const void *d_reqs;
  uint32_t n;
  uint32_t seg_cap;
  void *d_slots;
  void *d_cnt;      /* pack only */
  uint32_t *d_slot; /* [n]: written by pack, read by unpack */
  void *d_replies;  /* unpack only */
  const uint32_t *d_n; /* ABI v3: the batch's live request count in DEVICE memory (a batch a kernel produced -- the
                          GPU-resident clients -- whose size the host never sees), n is then its upper bound; NULL: n
                          is the count */
} dint_route_item;
int dint_route_pack_multi(const dint_route_item *items, uint32_t n_items, uint64_t seg_stride, uint64_t cnt_stride,
                          void *stream);
int dint_route_unpack_multi(const dint_route_item *items, uint32_t n_items, uint64_t seg_stride, void *stream);
/* n_seg segments of seg_cap message slots, segment k at d_base + k * seg_stride holding *(u32 *)(d_cnt + k *
 * cnt_stride) requests: processed in place as ONE serial history, segment by segment (kernel passes take whole
 * segments: seg_cap <= max_pass). */
int dint_submit_segments(dint_engine_t *e, void *d_base, uint32_t n_seg, uint32_t seg_cap, uint64_t seg_stride,
                         const void *d_cnt, uint64_t cnt_stride, void *stream);
/* (round 3; the config layout and DINT_ABI_VERSION are unchanged) the segments of SEVERAL engines (the shard servers of one GPU: same workload -- store, tatp or smallbank --
 * same device) answered by ONE set of kernel launches on ONE stream, the engines' kernels side by side in one grid.  A
 * closed-loop epoch or an exchange step hands every server its batch at the same moment; with one stream per engine that
 * is a fork and a join across streams per step, with this call it is three launches on the caller's stream (NULL: the
 * first engine's).  Every engine appears at most once in `items` (DINT_EINVAL otherwise).  Each engine's history is what dint_submit_segments would have produced.  Batches that do not fit one
 * kernel pass (n_seg * seg_cap > max_pass), lock / log engines, more than 4 items, and engines that do not agree in
 * DINT_FLAG_KV_ROUNDS, DINT_FLAG_KV_NO_HOT and DINT_FLAG_LOCK_SAME_KEY (one launch resolves every engine's hot keys the same
 * way) fall back to one dint_submit_segments per item on that stream; an announcement is then dropped. */
typedef struct dint_segments_item {
  dint_engine_t *engine;
  void *d_base;
  uint32_t n_seg, seg_cap;
  uint64_t seg_stride;
  const void *d_cnt;
  uint64_t cnt_stride;
} dint_segments_item;
int dint_submit_segments_multi(const dint_segments_item *items, uint32_t n_items, void *stream);
/* ... with a LOOK-AHEAD (round 6, as dint_submit_device_ahead): next[k] = the segments engine k will be handed by the NEXT call of
 * this kind -- the same engines in the same order, the same geometry (n_seg, seg_cap, strides), other buffers, complete in
 * device memory in the order of `stream` (the exchange has delivered them).  The engines' partitions of that step ride in this
 * step's launch set.  next == NULL, or an announcement that does not fit (other engines, another geometry, a workload without
 * the one-launch pass): plain dint_submit_segments_multi.  The announced step MUST be the engines' next submission: it is
 * answered by all of the engines or by none.  Anything else submitted to one of them in between fails with DINT_ESTATE as
 * after dint_submit_device_ahead and cancels the announcement of EVERY engine of the set (the others drop theirs when they
 * are next called); every engine of the set is then as if it had never seen the announced step (dint_submit_device_ahead: tail,
 * appended count, dint_stats, drain cursor; the ring slots from the tail on keep the step's records).  The announced buffers
 * hold what the first stage wrote (log requests answered in place): the step, if it is still wanted, is handed over again with
 * its requests. */
int dint_submit_segments_multi_ahead(const dint_segments_item *items, uint32_t n_items, const dint_segments_item *next, void *stream);
/* d_home[i] = home shard (0..shard_count-1) of d_reqs[i], computed on the GPU with the
 * same hash/modulus the engine uses; 0xFF for requests that have no home (bad table). */
int dint_home_shard(dint_engine_t *e, const void *d_reqs, uint32_t n, uint8_t *d_home, void *stream);

/* ---- measurement helpers -------------------------------------------------- */
/* Random 64-byte gather microbenchmark over `bytes` of HBM (roofline denominator,
 * SURVEY.md 8d): returns accesses per second via *out_aps, elapsed seconds via *out_s. */
int dint_bench_rand64(int32_t device, uint64_t bytes, uint64_t n_access, int write_back,
                      double *out_aps, double *out_s);
/* The general form: one access pattern over `bytes` of HBM, `blocks_per_cu` 256-thread workgroups per CU (0 = 8).
 * mode 0 = random gather of `width` (8 / 16 / 64) bytes from a 64-byte-aligned sector; 1 = the same + an 8-byte store
 * into the sector (read-modify-write); 2 = blind scatter of `width` (1 / 8 / 16 / 64) bytes; 3 = device-scope 64-bit
 * atomic add without / 4 = with a returned value; 5 / 6 = streaming read / write of the whole table in 16-byte
 * vectors (*out_aps = vectors per second).  Indices come from the engines' own hash + magic-multiply modulo. */
int dint_bench_access(int32_t device, uint64_t bytes, uint64_t n_access, uint32_t mode, uint32_t width,
                      uint32_t blocks_per_cu, double *out_aps, double *out_s);

/* Device primitives against their portable forms, on `device` (-1 = current): 0 = equal; bit 0 = the wave sort network
 * built from DPP / permlane exchanges differs from the ds_bpermute network, bit 1 = a single lane exchange differs;
 * negative = error.  (tests/test_gpu_locks.py; a diagnostic, not a hot-path call.) */
int dint_selftest(int32_t device);
/* Per-kernel launch time of the most recent dint_submit_device micro-batch sequence, measured
 * with HIP events on the stream the kernels ran on.  Call dint_timing_enable(e,1) first. */
int dint_timing_enable(dint_engine_t *e, int on);
/* returns number of kernels written; names[i] points to a static string */
int dint_timing_read(dint_engine_t *e, const char **names, double *avg_us, uint64_t *launches, int cap);

/* Debug (kv workloads, engine created with DINT_KV_TRACE=1 in the environment): per-wave timeline of the most
 * recent resolve launch, 16 u64 per bin: [0..9] s_memtime stamps (see k_kv.hip kv_stamp), [15] records in the bin.
 * Copies min(cap, 2048 * 16) words; returns the number of bins traced or DINT_ESTATE when tracing is off. */
int dint_kv_trace_read(dint_engine_t *e, uint64_t *out, uint64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* DINT_ABI_H */
