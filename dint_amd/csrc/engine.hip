// engine.hip -- host side of the C ABI (include/dint_abi.h): owns the HBM tables, the batch
// scratch, the streams, and turns dint_submit* into kernel launches.  Product path: there is no
// CPU fallback -- every entry point fails with DINT_ENODEV / DINT_EHIP when no gfx950 device works.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/dint_abi.h"
#include "dint_kernels.h"
#include "dint_kv.h"
#include "dint_populate.h"
#include "log_ring.h"
#include "state_load.h"
#include "state_rehash.h"
#include "state_stats.h"
#include "dint_traffic.h"

// k_locks.hip: one half of a lock pass (stage 1 = count + scan / place, 2 = resolve) on `st`
void dint_launch_lock_stage(uint32_t workload, int stage, const void *d_req, void *d_rep, uint32_t n, uint2 *table, dint_mod slots,
                            dint_shard shard, dint_scratch s, hipStream_t st, const dint_view &view);
// k_locks.hip: the resolve stage of a pass (set `s`) and the count stage of the next (set `sn`) in one launch; false = not possible
bool dint_launch_lock_fused(uint32_t workload, void *d_rep, uint32_t n, uint2 *table, dint_mod slots, dint_shard shard, dint_scratch s,
                            const dint_view &view, const void *next_req, void *next_rep, uint32_t next_n, dint_scratch sn,
                            const dint_view &next_view, hipStream_t st);

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess) return fail(DINT_EHIP, "%s: %s", #expr, hipGetErrorString(_e));  \
  } while (0)

const int kMsgSize[DINT_WL_COUNT] = {9, 6, 53, 53, 55, 23};

// kernel timing with HIP events on the stream the kernels run on
struct KernelTimer {
  static const int kMaxLaunch = 4096;
  bool on = false;
  int n_kernels = 0;             // kernels per pass (events per pass = n_kernels + 1)
  const char *names[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<hipEvent_t> ev;    // (n_kernels + 1) per recorded pass
  int passes = 0;
};

}  // namespace

struct dint_engine {
  dint_config cfg;
  uint32_t pass_max = DINT_MICRO;  // requests per kernel pass (<= the log ring size when a log is attached)
  int device = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;  // dint_submit* is serialised per engine: submission order = serial order
  uint32_t msg_size = 0;

  // batch scratch
  dint_scratch scratch{};
  dint_route_scratch route{};                              // dint_route_pack (allocated on first use)
  uint8_t *h_pinned = nullptr;                             // pinned buffer of dint_load_rows / dint_populate

  // host path: kNSlot staging slots {device request / reply buffers of one pass}; chunk k of a host submission
  // uses slot k % kNSlot, so the H2D copy of chunk k+1 and the D2H copy of chunk k-1 overlap the kernels of
  // chunk k (three streams, ordered by events).  Tickets are chunk sequence numbers.
  static const int kNSlot = 3;
  struct Slot {
    uint8_t *d_req = nullptr, *d_rep = nullptr;
    hipEvent_t h2d = nullptr, comp = nullptr, done = nullptr;
    uint64_t seq = 0;  // sequence number of the chunk that used the slot last (0 = never)
    // Pageable callers (a plain malloc / numpy buffer): hipMemcpyAsync never sees their memory.  The chunk is staged through
    // these page-locked buffers of the engine -- a host memcpy in on submission, a host memcpy out once the chunk has left
    // the GPU (at dint_wait, or when the slot is taken again).  r04: under rocprofv3 a pageable D2H / H2D of the HIP runtime
    // left the tail of a 4 KB page of one reply batch holding bytes of another (NOTEBOOK.md); the boundary contract
    // (lock_fasst/udp/net.h:33-48: the caller owns plain buffers) must not depend on the runtime's pageable path.
    uint8_t *h_req = nullptr, *h_rep = nullptr;
    uint8_t *deliver_to = nullptr;  // replies of the slot's chunk still to be copied from h_rep to the caller
    size_t deliver_bytes = 0;
  } slot[kNSlot];
  hipStream_t s_h2d = nullptr, s_d2h = nullptr;
  uint64_t next_seq = 1;
  uint64_t pool_seen = 0;  // pool_exhausted at the last host-path check
  unsigned long long *h_pool = nullptr;  // pinned: pool_exhausted counter read back with each host chunk

  // stream ordering: passes share one scratch set, so a pass enqueued on another stream than the previous one
  // first waits for it (dint_submit_device with a caller stream)
  hipStream_t last_stream = nullptr;
  hipEvent_t ev_order = nullptr;
  // ... the routing kernels have scratch of their own (route.blk) and touch neither tables nor pass
  // scratch: they are ordered among themselves only, so a pack for the next step overlaps the pass of this one
  hipStream_t route_last_stream = nullptr;
  hipEvent_t ev_route_order = nullptr;
  hipEvent_t ev_wait = nullptr, ev_signal = nullptr;  // dint_stream_wait / dint_stream_signal (re-recorded every call)

  // lock tables with DINT_FLAG_INPUTS_READY: the first half of pass k + 1 (k_lock_count, k_kv_scan_place: no table access) on
  // `helper` beside the second half of pass k; three scratch sets used in turn ([0] = `scratch`), an event pair per set
  struct LockPipe {
    static const int kSets = 3;
    bool ready = false;
    hipStream_t helper = nullptr;
    dint_scratch set[kSets];
    hipEvent_t counted[kSets] = {}, freed[kSets] = {}, ev_in = nullptr;
    bool used[kSets] = {};
    uint64_t seq = 0;
    bool after_serial = true;  // the previous pass ran on one stream (or there was none): the helper first waits for the caller's stream
  } lp;

  // lock tables (fasst / 2pl)
  uint2 *d_lock_tbl = nullptr;
  uint64_t n_slots = 0, n_local_slots = 0;
  dint_mod slots_mod{};

  // log
  dint_log log{};
  uint64_t log_drained = 0;  // records handed out (or given up as lost) by dint_log_drain
  uint64_t log_gone = 0;     // ... of them, lost to a cancelled announcement's records and not yet reported (log_ring.h)
  uint64_t snap_log_drained = 0;  // ... when the snapshot was taken (dint_restore puts it back)
  // log replay (dint_log_apply_device): scratch of one chunk, allocated on first use; the events of its stage timing
  dint_replay_scratch replay{};
  hipEvent_t ev_replay[4] = {};
  // log fold (dint_log_apply_folded_device): scratch of one chunk, allocated on first use; the events of its stage timing
  dint_fold_scratch fold{};
  hipEvent_t ev_fold[5] = {};
  // state sync (dint_state_digest / dint_state_diff / dint_state_repair): result words, and -- for the diff, in engine a --
  // the per-workgroup counts; allocated on first use
  dint_state_scratch state{};
  // block sync (dint_state_block_digest / _rows / _diff): result words, the digest's partials, the id list's and the lanes' arrays;
  // allocated on first use, grown to what a call needs and kept
  dint_block_scratch block{};
  // record routing (dint_records_route): the result words and the (shard, tile) counts with their scan; allocated on first use, grown
  // to what a call needs and kept
  dint_rroute_scratch rroute{};
  // table report (dint_state_stats): the workgroups' partial reports and the tables' reports, allocated on the first call
  dint_stats_scratch tstats{};
  // held locks (dint_state_locks / dint_state_unlock): the result words, the workgroups' counts, their scan and their partials;
  // allocated on first use, grown to what a call needs and kept
  dint_locks_scratch tlocks{};
  // table verify (dint_state_verify): the owner words, partial reports and reclaim arrays, allocated on the first call and kept
  dint_verify_scratch tverify{};
  hipEvent_t ev_verify[4] = {};  // with dint_timing_enable: before the chain stage, behind it, behind the lists, behind pool stage and sum
  // table compaction (dint_state_compact): row counts, scans and the staging buffers, allocated on the first call and kept
  dint_compact_scratch tcompact{};
  hipEvent_t ev_compact[5] = {};  // with dint_timing_enable: around the census, the count and its scans, the move, the commit
  // state image (dint_state_export / dint_state_import): scratch, grown on demand; `blank` = created or reset and since then
  // nothing but imports (what dint_state_import asks of its destination); the (source index, source count) pieces imported
  dint_image_scratch image{};
  bool blank = true;
  std::vector<std::pair<uint32_t, uint32_t>> pieces;
  // rehash (dint_state_rehash, in the destination): scratch, grown on demand and kept; the events of its stage timing
  dint_rehash_scratch rehash{};
  hipEvent_t ev_rehash[4 + 4 * DINT_KV_MAX_TABLES] = {};
  // bulk load (dint_load_rows_device / dint_populate_device): bit t of `fresh` = table t has taken nothing since creation / reset
  // (whatever clears `blank` clears every bit; a direct load clears its table's); scratch, grown on demand; the stage events
  uint32_t fresh = ~0u;
  dint_load_scratch load{};
  hipEvent_t ev_load[6] = {};

  // kv workloads (store / tatp / smallbank)
  dint_kv kv{};
  // look-ahead (r06, store / tatp): the batch whose partition stage ran inside the previous pass's k_kv_hot_part -- the
  // engine's next pass MUST be this one (its log records are in the ring, its records in the coarse bins)
  struct Ahead {
    bool valid = false;
    const void *req = nullptr;
    void *rep = nullptr;
    uint32_t n = 0;
    int set = 0;  // lock tables: the scratch set (0 = `scratch`, 1 = lp.set[1]) the announced batch's count stage filled
    uint32_t seg_cap = 0, n_seg = 0;  // a segmented batch (dint_submit_segments_multi_ahead): its geometry
    const void *cnt = nullptr;
    // a launch set's announcement: one word shared by the engines of the set.  The set is answered by all of them or by none,
    // so the first of them whose announcement is cancelled says so here, and the others drop theirs when they are next
    // looked at (ahead_settle)
    std::shared_ptr<std::atomic<bool>> broken;
  } ahead;

  // snapshot
  std::vector<std::pair<void *, size_t>> regions;  // device regions making up the engine state
  std::vector<void *> snap;

  dint_shard shard{0, 1};
  uint64_t batches = 0, requests = 0;
  KernelTimer timer;
};

namespace {

int dev_alloc(void **p, size_t bytes, bool zero = true) {
  hipError_t e = hipMalloc(p, bytes ? bytes : 1);
  if (e != hipSuccess) return fail(DINT_ENOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
  if (zero) {
    e = hipMemset(*p, 0, bytes);
    if (e != hipSuccess) return fail(DINT_EHIP, "hipMemset: %s", hipGetErrorString(e));
  }
  return 0;
}

void add_region(dint_engine *e, void *p, size_t bytes) { e->regions.push_back({p, bytes}); }

// Every enqueue on behalf of the engine goes through here: work on `st` is ordered after whatever the engine
// enqueued last on another stream.
int order_stream(dint_engine *e, hipStream_t st) {
  if (e->last_stream && e->last_stream != st) {
    // the engine's own stream outlives every call: its position is recorded now.  A CALLER's stream is never touched
    // after the call that used it (the caller may have destroyed it by now -- ADVICE r02): mark_stream recorded
    // ev_order on it at the end of that call.
    if (e->last_stream == e->stream) HIP_TRY(hipEventRecord(e->ev_order, e->stream));
    HIP_TRY(hipStreamWaitEvent(st, e->ev_order, 0));
  }
  e->last_stream = st;
  return 0;
}
int mark_stream(dint_engine *e, hipStream_t st) {  // end of a call that enqueued the engine's work on `st`
  if (st != e->stream) HIP_TRY(hipEventRecord(e->ev_order, st));
  return 0;
}

// The routing calls are ordered the same way, in a domain of their own: a caller's stream is never touched after the
// call that used it (mark_route_stream records ev_route_order on it before that call returns -- ADVICE r03).
int order_route_stream(dint_engine *e, hipStream_t st) {
  if (!e->ev_route_order) HIP_TRY(hipEventCreateWithFlags(&e->ev_route_order, hipEventDisableTiming));
  if (e->route_last_stream && e->route_last_stream != st) {
    if (e->route_last_stream == e->stream) HIP_TRY(hipEventRecord(e->ev_route_order, e->stream));
    HIP_TRY(hipStreamWaitEvent(st, e->ev_route_order, 0));
  }
  e->route_last_stream = st;
  return 0;
}
int mark_route_stream(dint_engine *e, hipStream_t st) {  // end of a routing call that enqueued on `st`
  if (st != e->stream && e->route_last_stream == st) HIP_TRY(hipEventRecord(e->ev_route_order, st));
  return 0;
}

int slot_alloc(dint_engine *e, int k) {
  dint_engine::Slot &sl = e->slot[k];
  if (sl.d_req) return 0;
  const size_t bytes = (size_t)e->pass_max * e->msg_size + 64;
  int rc = dev_alloc((void **)&sl.d_req, bytes, false);
  if (!rc) rc = dev_alloc((void **)&sl.d_rep, bytes, false);
  if (rc) return rc;
  HIP_TRY(hipEventCreateWithFlags(&sl.h2d, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&sl.comp, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
  return 0;
}

hipEvent_t *timer_events(dint_engine *e, int n_kernels, const char *const *names) {
  KernelTimer &t = e->timer;
  if (!t.on || t.passes >= KernelTimer::kMaxLaunch) return nullptr;
  t.n_kernels = n_kernels;
  for (int i = 0; i < n_kernels; i++) t.names[i] = names[i];
  size_t need = (size_t)(t.passes + 1) * (n_kernels + 1);
  while (t.ev.size() < need) {
    hipEvent_t ev;
    if (hipEventCreate(&ev) != hipSuccess) return nullptr;
    t.ev.push_back(ev);
  }
  hipEvent_t *p = &t.ev[(size_t)t.passes * (n_kernels + 1)];
  t.passes++;
  return p;
}

// kv passes: the tag of what the pieces of a hot key publish to each other in hotpub (k_kv.hip, kvh_word: 30 bits, never 0).
// When the counter wraps, the words are cleared on the pass's stream first, so a word left by the pass that carried the
// same tag 2^30 passes ago cannot be taken for this pass's.
int next_pass_seq(dint_engine *e, hipStream_t st) {
  e->scratch.kvs.pass_no++;  // (which set of the pass scratch a pass uses: dint_kv_sets)
  if (++e->scratch.pass_seq >= 0x3FFFFFFFu) {
    if (e->scratch.hotpub) HIP_TRY(hipMemsetAsync(e->scratch.hotpub, 0, (size_t)DINT_KV_HOTPUB_WORDS * sizeof(unsigned long long), st));
    if (e->scratch.kvs.bigrdy) HIP_TRY(hipMemsetAsync(e->scratch.kvs.bigrdy, 0, (size_t)DINT_KV_BIGQ_MAX * sizeof(uint32_t), st));
    e->scratch.pass_seq = 1;
  }
  return 0;
}
// kv engines: the log's ring position after the last pass lives in tail[(passes + 1) & 1] -- the partition of pass p reads
// tail[p & 1] and writes tail[(p + 1) & 1], because it may run beside the resolve stage of pass p - 1 (k_kv_pass), which used to
// copy one word onto the other.  dint_snapshot / dint_restore / dint_reset leave both words equal.
int log_cur(const dint_engine *e) { return e->kv.n_tables ? (int)lg_cur(e->scratch.kvs.pass_no) : 1; }

// one pass (n <= pass_max) on device buffers
// scratch sets 1 .. of the lock pipe: what k_lock_count / k_kv_scan_place / k_lock_resolve share within one pass
int lock_pipe_init(dint_engine *e) {
  dint_engine::LockPipe &lp = e->lp;
  if (lp.ready) return 0;
  // (a call after a failed one -- an allocation that did not fit -- must not create streams, events or buffers a second time)
  if (!lp.helper) HIP_TRY(hipStreamCreateWithFlags(&lp.helper, hipStreamNonBlocking));
  if (!lp.ev_in) HIP_TRY(hipEventCreateWithFlags(&lp.ev_in, hipEventDisableTiming));
  for (int k = 0; k < dint_engine::LockPipe::kSets; k++) {
    if (!lp.counted[k]) HIP_TRY(hipEventCreateWithFlags(&lp.counted[k], hipEventDisableTiming));
    if (!lp.freed[k]) HIP_TRY(hipEventCreateWithFlags(&lp.freed[k], hipEventDisableTiming));
    if (k == 0) continue;  // set 0 is e->scratch itself
    dint_scratch &s = lp.set[k];
    if (s.stats) {  // a set an earlier, failed call began: what it got is given back first
      const dint_scratch &o = e->scratch;
      if (s.bin_cnt != o.bin_cnt) hipFree(s.bin_cnt);
      if (s.bins != o.bins) hipFree(s.bins);
      if (s.blk_pub != o.blk_pub && s.blk_pub != o.blk_pub_next && s.blk_pub_next != o.blk_pub) hipFree(std::min(s.blk_pub, s.blk_pub_next));
      if (s.big != o.big && s.big != o.big_next && s.big_next != o.big) hipFree(std::min(s.big, s.big_next));
      if (s.bin_off != o.bin_off) hipFree(s.bin_off);
      if (s.ovl != o.ovl) hipFree(s.ovl);
      if (s.ovf != o.ovf) hipFree(s.ovf);
      if (s.kbins != o.kbins) hipFree(s.kbins);
    }
    s = e->scratch;  // (stats, lock_trace: shared)
    int rc = dev_alloc((void **)&s.bin_cnt, DINT_KV_PMAX * sizeof(uint32_t));
    if (!rc) rc = dev_alloc((void **)&s.bins, (size_t)DINT_KV_PMAX * DINT_KV_BINCAP * sizeof(uint64_t), false);
    if (!rc) rc = dev_alloc((void **)&s.blk_pub, 2 * 1024 * sizeof(uint32_t));
    if (!rc) rc = dev_alloc((void **)&s.big, 2 * (4 + DINT_KV_PMAX) * sizeof(uint32_t));
    if (!rc) rc = dev_alloc((void **)&s.bin_off, DINT_KV_PMAX * sizeof(uint32_t));
    if (!rc && hipMemset(s.bin_off, 0xFF, DINT_KV_PMAX * sizeof(uint32_t)) != hipSuccess) rc = fail(DINT_EHIP, "hipMemset");
    if (!rc && e->scratch.kbins) rc = dev_alloc((void **)&s.kbins, (size_t)e->scratch.kbins_slots * sizeof(uint64_t), false);
    if (!rc) rc = dev_alloc((void **)&s.ovl, (size_t)e->pass_max * sizeof(uint4), false);
    if (!rc) rc = dev_alloc((void **)&s.ovf, (size_t)e->pass_max * sizeof(uint64_t), false);
    if (rc) return rc;
    s.blk_pub_next = s.blk_pub + 1024;
    s.big_next = s.big + (4 + DINT_KV_PMAX);
  }
  // The zero fills above ran on the NULL stream, which the helper stream and the engine's own (non-blocking) do not wait for: the
  // first count stage on a new set could find its counters and region names not yet cleared.  Never seen in a plain run (the fills
  // take microseconds); under `rocprofv3 --pmc`, which serializes every dispatch, it was `k_lock_count`'s trap and wrong replies of
  // the DINT_FLAG_INPUTS_READY engine (r06, NOTEBOOK.md).
  HIP_TRY(hipDeviceSynchronize());
  lp.ready = true;
  return 0;
}
void lock_pipe_destroy(dint_engine *e) {
  dint_engine::LockPipe &lp = e->lp;
  if (lp.helper) { hipStreamSynchronize(lp.helper); hipStreamDestroy(lp.helper); }
  if (lp.ev_in) hipEventDestroy(lp.ev_in);
  for (int k = 0; k < dint_engine::LockPipe::kSets; k++) {
    if (lp.counted[k]) hipEventDestroy(lp.counted[k]);
    if (lp.freed[k]) hipEventDestroy(lp.freed[k]);
    if (k == 0) continue;
    // (whatever lock_pipe_init got before a failed allocation is freed too: a set's pointers start as copies of the engine's own
    // and are replaced one by one -- only the replaced ones are this set's)
    dint_scratch &s = lp.set[k];
    const dint_scratch &o = e->scratch;
    if (s.bin_cnt != o.bin_cnt) hipFree(s.bin_cnt);
    if (s.bins != o.bins) hipFree(s.bins);
    if (s.blk_pub != o.blk_pub && s.blk_pub != o.blk_pub_next && s.blk_pub_next != o.blk_pub) hipFree(std::min(s.blk_pub, s.blk_pub_next));
    if (s.big != o.big && s.big != o.big_next && s.big_next != o.big) hipFree(std::min(s.big, s.big_next));
    if (s.bin_off != o.bin_off) hipFree(s.bin_off);
    if (s.ovl != o.ovl) hipFree(s.ovl);
    if (s.ovf != o.ovf) hipFree(s.ovf);
    if (s.kbins != o.kbins) hipFree(s.kbins);
  }
}
// a lock pass in two halves (DINT_FLAG_INPUTS_READY, dint_submit_device): count + scan / place on the helper stream as soon
// as the scratch set is free, resolve on the caller's stream behind it -- and behind the previous pass's resolve, which owns
// the table.  `st` has been ordered behind the previous pass's stream already (order_stream).
int run_lock_pass_piped(dint_engine *e, const void *d_req, uint32_t n, void *d_rep, hipStream_t st, const dint_view &view) {
  if (int rc = lock_pipe_init(e)) return rc;
  dint_engine::LockPipe &lp = e->lp;
  const int b = (int)(lp.seq++ % dint_engine::LockPipe::kSets);
  dint_scratch &s = b == 0 ? e->scratch : lp.set[b];
  if (lp.after_serial) {  // whatever ran on one stream before (a pass with timing on, a restore, the first call): behind it
    HIP_TRY(hipEventRecord(lp.ev_in, st));
    HIP_TRY(hipStreamWaitEvent(lp.helper, lp.ev_in, 0));
    lp.after_serial = false;
  }
  if (lp.used[b]) HIP_TRY(hipStreamWaitEvent(lp.helper, lp.freed[b], 0));  // the resolve that read this set last
  dint_launch_lock_stage(e->cfg.workload, 1, d_req, d_rep, n, e->d_lock_tbl, e->slots_mod, e->shard, s, lp.helper, view);
  HIP_TRY(hipEventRecord(lp.counted[b], lp.helper));
  HIP_TRY(hipStreamWaitEvent(st, lp.counted[b], 0));
  dint_launch_lock_stage(e->cfg.workload, 2, d_req, d_rep, n, e->d_lock_tbl, e->slots_mod, e->shard, s, st, view);
  HIP_TRY(hipEventRecord(lp.freed[b], st));
  lp.used[b] = true;
  std::swap(s.big, s.big_next);  // the big-bin lists alternate between the passes of a set
  std::swap(s.blk_pub, s.blk_pub_next);
  return 0;
}

// An announced batch (dint_submit_device_ahead) that will not be submitted after all: its partition stage has filled the
// coarse bins and the control words of the next pass -- drain the GPU and leave the pass scratch as between passes.  What
// the stage wrote outside the scratch is taken back too (include/dint_abi.h: the engine is as if it had never seen the batch):
// the log's tail, appended count and drain cursor (log_ring.h, lg_cancel) and the bad / foreign requests it counted into
// dint_stats -- by the counts the partition left in the announced pass's control words (DINT_KV_CTL_LOGN ..).  The ring slots
// from the tail on keep the batch's records: the one thing that stays.
int ahead_cancel(dint_engine *e) {
  if (!e->ahead.valid) return 0;
  e->ahead.valid = false;
  if (e->ahead.broken) e->ahead.broken->store(true);
  e->ahead.broken.reset();
  HIP_TRY(hipDeviceSynchronize());
  if (!e->kv.n_tables) {  // a lock engine: the counters, the big-bin list and the region names of the set the count stage filled
    dint_scratch &ls = e->ahead.set == 0 ? e->scratch : e->lp.set[e->ahead.set];
    HIP_TRY(hipMemset(ls.bin_cnt, 0, DINT_KV_PMAX * sizeof(uint32_t)));
    HIP_TRY(hipMemset(std::min(ls.big, ls.big_next), 0, 2 * (4 + DINT_KV_PMAX) * sizeof(uint32_t)));
    HIP_TRY(hipMemset(ls.bin_off, 0xFF, DINT_KV_PMAX * sizeof(uint32_t)));
    HIP_TRY(hipDeviceSynchronize());  // (the fills ran on the null stream: the engine's streams do not wait for it)
    return 0;
  }
  dint_scratch &s = e->scratch;
  // what the cancelled partition counted, before its control words are cleared: {log records, bad requests, foreign requests}
  // (the announced pass is number pass_no + 1: it was never launched)
  uint32_t cnt[3];
  static_assert(DINT_KV_CTL_BAD == DINT_KV_CTL_LOGN + 1 && DINT_KV_CTL_FOREIGN == DINT_KV_CTL_LOGN + 2, "three words in a row");
  HIP_TRY(hipMemcpy(cnt, s.kvs.ctl[(s.kvs.pass_no + 1) % 3] + DINT_KV_CTL_LOGN, sizeof cnt, hipMemcpyDeviceToHost));
  for (int k = 0; k < 2; k++) HIP_TRY(hipMemset(s.kvs.bin_cnt[k], 0, DINT_KV_PMAX * sizeof(uint32_t)));
  HIP_TRY(hipMemset(s.kvs.ctl[0], 0, 3 * DINT_KV_CTL_WORDS * sizeof(uint32_t)));
  HIP_TRY(hipMemset(s.kvs.pub[0], 0, 3 * 1024 * sizeof(uint32_t)));
  if (e->log.tail) {  // the tail the cancelled partition published is not the current one
    uint32_t t[4];
    HIP_TRY(hipMemcpy(t, e->log.tail, sizeof t, hipMemcpyDeviceToHost));
    const uint32_t c = (uint32_t)log_cur(e);  // (the cancelled pass was never counted: `c` is the word it read, c ^ 1 the one it wrote)
    LgRing r = {{t[0], t[1]}, (uint64_t)t[2] | ((uint64_t)t[3] << 32), e->log_drained, e->log_gone};
    lg_cancel(r, c, cnt[0], e->log.cap);
    t[0] = r.tail[0]; t[1] = r.tail[1]; t[2] = (uint32_t)r.appended; t[3] = (uint32_t)(r.appended >> 32);
    e->log_drained = r.drained; e->log_gone = r.gone;
    HIP_TRY(hipMemcpy(e->log.tail, t, sizeof t, hipMemcpyHostToDevice));
  }
  if (cnt[1] || cnt[2]) {  // (rare: malformed requests, requests of another shard)
    unsigned long long v[2];
    HIP_TRY(hipMemcpy(&v[0], &s.stats->bad_requests, sizeof v[0], hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&v[1], &s.stats->foreign_requests, sizeof v[1], hipMemcpyDeviceToHost));
    v[0] -= std::min<unsigned long long>(v[0], cnt[1]);
    v[1] -= std::min<unsigned long long>(v[1], cnt[2]);
    HIP_TRY(hipMemcpy(&s.stats->bad_requests, &v[0], sizeof v[0], hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(&s.stats->foreign_requests, &v[1], sizeof v[1], hipMemcpyHostToDevice));
  }
  HIP_TRY(hipDeviceSynchronize());  // (the fills ran on the null stream: the engine's streams do not wait for it)
  return 0;
}

// An engine of a launch set whose announcement another engine of the set has cancelled: the set will not be answered as
// announced, so this engine's share of it is cancelled too, silently (the caller that broke the set was told).
int ahead_settle(dint_engine *e) {
  if (!e->ahead.valid || !e->ahead.broken || !e->ahead.broken->load()) return 0;
  HIP_TRY(hipSetDevice(e->device));  // (some callers look before they have chosen the device)
  return ahead_cancel(e);
}

int run_pass(dint_engine *e, const void *d_req, uint32_t n, void *d_rep, hipStream_t st, int load_mode = 0,
             const dint_view &view = dint_flat_view(), bool inputs_ready = false, const dint_kv_ahead *next = nullptr) {
  bool part_done = false;
  e->blank = false, e->fresh = 0;
  if (int rc = ahead_settle(e)) return rc;
  if (e->ahead.valid) {  // the pass that was announced, and nothing else
    if (e->ahead.req != d_req || e->ahead.rep != d_rep || e->ahead.n != n || view.seg_cap != e->ahead.seg_cap || load_mode) {
      if (int rc = ahead_cancel(e)) return rc;
      return fail(DINT_ESTATE, "the batch announced by dint_submit_device_ahead (%u requests at %p) must be the engine's next "
                               "submission; the announcement is cancelled", e->ahead.n, e->ahead.req);
    }
    e->ahead.valid = false;
    e->ahead.broken.reset();
    part_done = true;
  }
  if (int rc = order_stream(e, st)) return rc;
  bool piped = inputs_ready && n && !e->timer.on && (e->cfg.workload == DINT_WL_FASST || e->cfg.workload == DINT_WL_2PL);
  if (piped && part_done) {
    // the pass was announced by one that was not piped (kernel timing was on then): its count stage has run, into e->ahead.set.
    // The piped path would count it again, into a set of its own rotation -- after one earlier piped pass the same set.  This
    // pass resolves from the set it was counted into, on one stream, and announces nothing: the next one is piped again.
    piped = false;
    next = nullptr;
  }
  if (!piped) e->lp.after_serial = true;
  static const char *const lock_names[] = {"k_lock_count", "k_kv_scan_place", "k_lock_resolve"};
  static const char *const log_names[] = {"k_log_append"};
  static const char *const kv_names[] = {"k_kv_part", "k_kv_resolve", "k_kv_hot", "k_kv_big"};
  static const char *const kv_names_one[] = {"k_kv_part", "k_kv_pass", "k_kv_late"};  // (store / tatp, r06: one launch per pass + the late list's)
  switch (piped ? DINT_WL_COUNT : e->cfg.workload) {
    case DINT_WL_COUNT:
      if (int rc = run_lock_pass_piped(e, d_req, n, d_rep, st, view)) return rc;
      break;
    case DINT_WL_FASST:
    case DINT_WL_2PL: {
      // r06: with the next batch announced (or the next slice of one long submission), this pass's resolve stage and the next
      // pass's count stage are ONE launch (k_lock_pass) -- two scratch sets used in turn, `scratch` and lp.set[1]
      const int b = part_done ? e->ahead.set : 0;
      if (next && (!n || !next->n || view.seg_cap || next->view.seg_cap || n > DINT_MICRO_BATCH || next->n > DINT_MICRO_BATCH ||
                   !e->scratch.kbins || getenv("DINT_LOCK_NO_FUSE")))
        next = nullptr;
      if ((next || b) && !e->lp.ready)
        if (int rc = lock_pipe_init(e)) return rc;
      dint_scratch &s = b == 0 ? e->scratch : e->lp.set[b];
      hipEvent_t *ev = timer_events(e, 3, lock_names);
      if (!part_done && !next) {
        if (e->cfg.workload == DINT_WL_FASST) dint_launch_fasst(d_req, d_rep, n, e->d_lock_tbl, e->slots_mod, e->shard, s, st, ev, view);
        else dint_launch_2pl(d_req, d_rep, n, e->d_lock_tbl, e->slots_mod, e->shard, s, st, ev, view);
      } else {
        if (ev) HIP_TRY(hipEventRecord(ev[0], st));
        if (!part_done) dint_launch_lock_stage(e->cfg.workload, 1, d_req, d_rep, n, e->d_lock_tbl, e->slots_mod, e->shard, s, st, view);
        if (ev) { HIP_TRY(hipEventRecord(ev[1], st)); HIP_TRY(hipEventRecord(ev[2], st)); }
        dint_scratch &sn = b == 0 ? e->lp.set[1] : e->scratch;
        if (!next || !dint_launch_lock_fused(e->cfg.workload, d_rep, n, e->d_lock_tbl, e->slots_mod, e->shard, s, view, next->d_req, next->d_rep,
                                             next->n, sn, next->view, st)) {
          dint_launch_lock_stage(e->cfg.workload, 2, d_req, d_rep, n, e->d_lock_tbl, e->slots_mod, e->shard, s, st, view);
          next = nullptr;
        }
        if (ev) HIP_TRY(hipEventRecord(ev[3], st));
      }
      std::swap(s.big, s.big_next);  // the big-bin lists alternate between the passes of a set
      std::swap(s.blk_pub, s.blk_pub_next);
      if (next) {
        e->ahead.valid = true;
        e->ahead.req = next->d_req; e->ahead.rep = next->d_rep; e->ahead.n = next->n;
        e->ahead.set = b ^ 1;
        e->ahead.seg_cap = 0; e->ahead.n_seg = 0; e->ahead.cnt = nullptr;
      }
      break;
    }
    case DINT_WL_LOG:
      if (view.seg_cap) return fail(DINT_ESTATE, "the log workload is not sharded by key");
      dint_launch_log(d_req, d_rep, n, e->log, e->scratch, st, timer_events(e, 1, log_names));
      std::swap(e->scratch.blk_pub, e->scratch.blk_pub_next);  // the tile counts alternate between passes
      break;
    case DINT_WL_STORE:
    case DINT_WL_TATP:
    case DINT_WL_SMALLBANK:
      if (int rc = next_pass_seq(e, st)) return rc;  // tags what the pieces of a hot key publish in this pass
      if (next && (!n || !next->n || view.seg_cap || next->view.seg_cap || !dint_kv_ahead_ok(e->kv, load_mode))) next = nullptr;
      dint_launch_kv(d_req, d_rep, n, e->kv, e->log, e->scratch, load_mode, st,
                     dint_kv_one_launch(e->kv, load_mode) ? timer_events(e, 3, kv_names_one) : timer_events(e, 4, kv_names), view, part_done, next);
      if (next) {
        e->ahead.valid = true;
        e->ahead.req = next->d_req; e->ahead.rep = next->d_rep; e->ahead.n = next->n;
        e->ahead.seg_cap = 0; e->ahead.n_seg = 0; e->ahead.cnt = nullptr;
        e->ahead.broken.reset();
      }
      break;
    default:
      return fail(DINT_EINVAL, "bad workload");
  }
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(DINT_EHIP, "kernel launch: %s", hipGetErrorString(err));
  if (int rc = mark_stream(e, st)) return rc;
  e->batches++;
  e->requests += n;
  return 0;
}

// bulk load (kvs_insert semantics, explicit version) = passes of internal LOAD requests through the
// same scatter/resolve kernels, so rows land in request order exactly like wire INSERTs
int load_rows_locked(dint_engine *e, uint32_t table, const uint64_t *keys, const uint32_t *vers, const uint8_t *vals,
                     uint64_t n) {
  const dint_kv_fmt f = dint_kv_format(e->cfg.workload);
  for (uint64_t off = 0; off < n; off += e->pass_max) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(e->pass_max, n - off);
    const size_t bytes = (size_t)m * f.msg;
    memset(e->h_pinned, 0, bytes);
    for (uint32_t i = 0; i < m; i++) {
      uint8_t *msg = e->h_pinned + (size_t)i * f.msg;
      msg[f.type] = (uint8_t)DINT_KV_LOAD_OP;
      if (f.table != 0xFFFFFFFFu) msg[f.table] = (uint8_t)table;
      memcpy(msg + f.key, &keys[off + i], 8);
      memcpy(msg + f.val, vals + (off + i) * f.val_size, f.val_size);
      const uint32_t ver = vers ? vers[off + i] : 0;
      memcpy(msg + f.ver, &ver, 4);
    }
    if (int rc = order_stream(e, e->stream)) return rc;
    HIP_TRY(hipMemcpyAsync(e->slot[0].d_req, e->h_pinned, bytes, hipMemcpyHostToDevice, e->stream));
    if (int rc = run_pass(e, e->slot[0].d_req, m, e->slot[0].d_req, e->stream, 1)) return rc;
    e->batches--;  // population passes are not request batches
    e->requests -= m;
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  return 0;
}

// log replay scratch: everything a chunk of `cap` records needs (dint_kernels.h dint_replay_scratch)
void replay_free(dint_engine *e) {
  dint_replay_scratch &r = e->replay;
  hipFree(r.row_in); hipFree(r.row_out); hipFree(r.idx_in); hipFree(r.idx_out); hipFree(r.slot); hipFree(r.types);
  hipFree(r.sort_tmp); hipFree(r.probe); hipFree(r.msgs); hipFree(r.probe_n); hipFree(r.counts);
  r = dint_replay_scratch{};
}
int replay_alloc(dint_engine *e, uint32_t cap) {
  dint_replay_scratch &r = e->replay;
  if (r.cap >= cap) return 0;
  HIP_TRY(hipStreamSynchronize(e->stream));  // (a replay that still uses the smaller set)
  replay_free(e);
  const bool tatp = e->cfg.workload == DINT_WL_TATP;
  int rc = dev_alloc((void **)&r.msgs, (size_t)cap * e->msg_size + 64, false);
  if (!rc) rc = dev_alloc((void **)&r.counts, 4 * sizeof(unsigned long long));
  if (!rc) rc = dev_alloc((void **)&r.probe_n, 4 * sizeof(uint32_t));
  if (!rc && tatp) {
    const int64_t tmp = dint_replay_sort_bytes(cap, e->stream);
    if (tmp < 0) rc = fail(DINT_EHIP, "radix sort: temporary storage query failed");
    if (!rc) rc = dev_alloc((void **)&r.row_in, (size_t)cap * sizeof(uint64_t), false);
    if (!rc) rc = dev_alloc((void **)&r.row_out, (size_t)cap * sizeof(uint64_t), false);
    if (!rc) rc = dev_alloc((void **)&r.idx_in, (size_t)cap * sizeof(uint32_t), false);
    if (!rc) rc = dev_alloc((void **)&r.idx_out, (size_t)cap * sizeof(uint32_t), false);
    if (!rc) rc = dev_alloc((void **)&r.slot, (size_t)cap * sizeof(uint32_t), false);
    if (!rc) rc = dev_alloc((void **)&r.types, cap, false);
    if (!rc) rc = dev_alloc(&r.sort_tmp, (size_t)tmp, false);
    if (!rc) rc = dev_alloc((void **)&r.probe, (size_t)std::max(cap, 2u) * e->msg_size + 64, false);
    r.sort_tmp_bytes = (size_t)std::max<int64_t>(tmp, 0);
  }
  if (rc) {
    replay_free(e);
    return rc;
  }
  HIP_TRY(hipDeviceSynchronize());  // (the zero fills ran on the null stream: the engine's stream does not wait for it)
  r.cap = cap;
  return 0;
}

// log fold scratch: everything a chunk of `cap` records needs (dint_kernels.h dint_fold_scratch)
void fold_free(dint_engine *e) {
  dint_fold_scratch &f = e->fold;
  void *all[] = {f.k0, f.k1, f.i0, f.i1, f.place_log, f.key_s, f.del_s, f.flag, f.delpos, f.rowid, f.lastdel, f.row_start, f.row_occ,
                 f.row_v0, f.row_kind, f.row_ver, f.row_defer, f.has, f.epos, f.dflag, f.dpos, f.repair, f.def_rec, f.tmp, f.words,
                 f.counts};
  for (void *p : all) hipFree(p);
  f = dint_fold_scratch{};
}
int fold_alloc(dint_engine *e, uint32_t cap) {
  dint_fold_scratch &f = e->fold;
  if (f.cap >= cap) return 0;
  HIP_TRY(hipStreamSynchronize(e->stream));  // (a call that still uses the smaller set)
  fold_free(e);
  const int64_t tmp = dint_fold_tmp_bytes(cap, e->stream);
  if (tmp < 0) return fail(DINT_EHIP, "log fold: temporary storage query failed");
  const size_t n = cap;
  int rc = 0;
  auto get = [&](auto **p, size_t bytes, bool zero = false) {
    if (!rc) rc = dev_alloc((void **)p, bytes, zero);
  };
  get(&f.k0, n * 8); get(&f.k1, n * 8); get(&f.i0, n * 4); get(&f.i1, n * 4); get(&f.place_log, n * 8); get(&f.key_s, n * 8);
  get(&f.del_s, n); get(&f.flag, n * 4); get(&f.delpos, n * 4); get(&f.rowid, n * 4); get(&f.lastdel, n * 4);
  get(&f.row_start, (n + 1) * 4); get(&f.row_occ, n * 4); get(&f.row_v0, n * 4); get(&f.row_kind, n * 4); get(&f.row_ver, n * 4);
  get(&f.row_defer, n); get(&f.has, n * 4); get(&f.epos, n * 4); get(&f.dflag, n * 4); get(&f.dpos, n * 4);
  get(&f.repair, n * 64); get(&f.def_rec, n * 64); get(&f.tmp, (size_t)tmp);
  get(&f.words, 4 * sizeof(uint32_t), true); get(&f.counts, DINT_FOLD_COUNTS * sizeof(unsigned long long), true);
  f.tmp_bytes = (size_t)tmp;
  if (rc) {
    fold_free(e);
    return rc;
  }
  HIP_TRY(hipDeviceSynchronize());  // (the zero fills ran on the null stream: the engine's stream does not wait for it)
  f.cap = cap;
  return 0;
}

// state sync scratch: the result words always, the diff's per-workgroup arrays when asked for
void state_free(dint_engine *e) {
  hipFree(e->state.words); hipFree(e->state.blk_cnt); hipFree(e->state.blk_off); hipFree(e->state.digest_part);
  e->state = dint_state_scratch{};
}
int state_alloc(dint_engine *e, bool diff) {
  dint_state_scratch &s = e->state;
  bool fresh = false;
  if (!s.words) {
    if (int rc = dev_alloc((void **)&s.words, DINT_STATE_WORDS * sizeof(unsigned long long))) return rc;
    fresh = true;
  }
  if (!s.digest_part) {
    if (int rc = dev_alloc((void **)&s.digest_part, (size_t)DINT_KV_MAX_TABLES * DINT_STATE_DIGEST_GRID * 4 * sizeof(unsigned long long), false))
      return rc;
  }
  if (diff && !s.nb) {
    const uint32_t nb = dint_state_blocks(e->kv);
    int rc = dev_alloc((void **)&s.blk_cnt, (size_t)nb * sizeof(uint32_t));
    if (!rc) rc = dev_alloc((void **)&s.blk_off, (size_t)nb * sizeof(uint64_t));
    if (rc) {
      hipFree(s.blk_cnt); hipFree(s.blk_off);
      s.blk_cnt = nullptr; s.blk_off = nullptr;
      return rc;
    }
    s.nb = nb;
    fresh = true;
  }
  if (fresh) HIP_TRY(hipDeviceSynchronize());  // (the zero fills ran on the null stream: the engine's stream does not wait for it)
  return 0;
}
// block sync scratch: every array grows to what a call needs and is kept (no zero fill: every call clears what it reads)
void block_free(dint_engine *e) {
  dint_block_scratch &s = e->block;
  hipFree(s.words); hipFree(s.part); hipFree(s.id_cnt); hipFree(s.id_off); hipFree(s.blk_cnt); hipFree(s.blk_off); hipFree(s.run_lo); hipFree(s.run_hi);
  s = dint_block_scratch{};
}
int block_reserve(dint_engine *e, uint64_t chunks, uint64_t ids, uint64_t lanes, bool runs) {
  dint_block_scratch &s = e->block;
  auto grow = [](void **a, size_t sa, void **b, size_t sb, uint64_t &have, uint64_t need) -> int {
    if (need <= have) return 0;
    hipFree(*a); hipFree(*b);
    *a = *b = nullptr;
    have = 0;
    int rc = dev_alloc(a, (size_t)need * sa, false);
    if (!rc) rc = dev_alloc(b, (size_t)need * sb, false);
    if (rc) {
      hipFree(*a); hipFree(*b);
      *a = *b = nullptr;
      return rc;
    }
    have = need;
    return 0;
  };
  if (!s.words)
    if (int rc = dev_alloc((void **)&s.words, DINT_BLOCK_WORDS * sizeof(unsigned long long), false)) return rc;
  if (chunks > s.part_n) {
    hipFree(s.part);
    s.part = nullptr;
    s.part_n = 0;
    if (int rc = dev_alloc((void **)&s.part, (size_t)chunks * 4 * sizeof(unsigned long long), false)) return rc;
    s.part_n = chunks;
  }
  if (int rc = grow((void **)&s.id_cnt, sizeof(uint32_t), (void **)&s.id_off, sizeof(uint64_t), s.id_n, ids)) return rc;
  if (int rc = grow((void **)&s.blk_cnt, sizeof(uint32_t), (void **)&s.blk_off, sizeof(uint64_t), s.blk_n, (lanes + 255) / 256)) return rc;
  if (runs)
    if (int rc = grow((void **)&s.run_lo, sizeof(uint32_t), (void **)&s.run_hi, sizeof(uint32_t), s.run_n, lanes)) return rc;
  return 0;
}
int state_launched();
// record routing scratch: grows to what a call needs and is kept (no zero fill: every call writes what it reads)
void rroute_free(dint_engine *e) {
  dint_rroute_scratch &s = e->rroute;
  hipFree(s.words); hipFree(s.cnt); hipFree(s.off);
  s = dint_rroute_scratch{};
}
int rroute_reserve(dint_engine *e, uint64_t counts) {
  dint_rroute_scratch &s = e->rroute;
  if (!s.words)
    if (int rc = dev_alloc((void **)&s.words, DINT_RROUTE_WORDS * sizeof(unsigned long long), false)) return rc;
  if (counts <= s.cnt_n) return 0;
  hipFree(s.cnt); hipFree(s.off);
  s.cnt = nullptr; s.off = nullptr; s.cnt_n = 0;
  int rc = dev_alloc((void **)&s.cnt, (size_t)counts * sizeof(uint32_t), false);
  if (!rc) rc = dev_alloc((void **)&s.off, (size_t)counts * sizeof(uint64_t), false);
  if (rc) {
    hipFree(s.cnt); hipFree(s.off);
    s.cnt = nullptr; s.off = nullptr;
    return rc;
  }
  s.cnt_n = counts;
  return 0;
}
// a shard of a replica set (DINT_FLAG_SHARD_REPLICA): it places records at their local bucket and refuses foreign ones
bool shard_replica(const dint_engine *e) { return e->shard.count > 1 && (e->cfg.flags & DINT_FLAG_SHARD_REPLICA) != 0; }
// the checks the three state calls share for one engine, before any GPU work
int state_check(const dint_engine *e, bool sharded_ok) {
  if (!e->kv.n_tables) return fail(DINT_ESTATE, "workload has no kv table");
  if (!sharded_ok && e->shard.count > 1 && !shard_replica(e)) return fail(DINT_EINVAL, "a sharded engine: rows are not routed here");
  return 0;
}
// a flagged shard before a log replay: all n records are read once, and a record of another shard or of no table refuses the list
// (on the engine's stream, already ordered; one synchronisation)
int shard_home_check(dint_engine *e, const void *d_records, uint64_t n, hipStream_t st) {
  if (int rc = state_alloc(e, false)) return rc;
  dint_launch_state_home_check(e->kv, d_records, n, e->state, st);
  if (int rc = state_launched()) return rc;
  unsigned long long bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, e->state.words + DINT_STATE_HOME_AT, sizeof bad, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return bad ? fail(DINT_EINVAL, "a record is home to another shard or names a table the workload has not (dint_records_route makes a "
                                 "shard's piece); nothing was applied")
             : 0;
}
// ... under the engine's mutex: the state calls read the tables where they lie, so none runs between an announcement and its pass
int state_quiet(dint_engine *e) {
  if (int rc = ahead_settle(e)) return rc;
  return e->ahead.valid ? fail(DINT_ESTATE, "a batch announced by dint_submit_device_ahead is pending") : 0;
}
// ... after a launcher
int state_launched() {
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : fail(DINT_EHIP, "kernel launch: %s", hipGetErrorString(err));
}

// held locks: the engine's lock units as the launchers take them, and the scratch (grown to nb workgroups and kept)
void locks_free(dint_engine *e) {
  hipFree(e->tlocks.words); hipFree(e->tlocks.cnt); hipFree(e->tlocks.off); hipFree(e->tlocks.part);
  e->tlocks = dint_locks_scratch{};
}
int locks_view(const dint_engine *e, dint_locks_view *v) {
  memset(v, 0, sizeof *v);
  lk_geom &g = v->g;
  g.mode = lk_mode(e->cfg.workload);
  if (g.mode == LK_NONE) return fail(DINT_ESTATE, "workload has no lock table");
  g.shard_index = e->shard.index; g.shard_count = e->shard.count ? e->shard.count : 1;
  if (lk_is_kv(g.mode)) {
    g.n_tables = e->kv.n_tables;
    g.same_key = e->kv.h.same_key;
    for (uint32_t t = 0; t < g.n_tables; t++) {
      v->tab[t] = e->kv.h.tab[t];
      v->lockmod[t] = e->kv.h.lockmod[t];
      g.n_local[t] = e->kv.h.tab[t].n_local;
      g.size[t] = e->kv.hash_size[t];
    }
  } else {
    g.n_tables = 1;
    g.n_local[0] = e->n_local_slots;
    g.size[0] = e->n_slots;
    v->tbl = e->d_lock_tbl;
  }
  return 0;
}
int locks_reserve(dint_engine *e, uint64_t nb) {
  dint_locks_scratch &s = e->tlocks;
  if (!s.words)
    if (int rc = dev_alloc((void **)&s.words, DINT_LOCKS_WORDS * sizeof(unsigned long long), false)) return rc;  // (every word a call reads it has written on its stream)
  if (nb <= s.nb) return 0;
  hipFree(s.cnt); hipFree(s.off); hipFree(s.part);  // (waits for the device: nothing of an earlier call still reads them)
  s.cnt = nullptr; s.off = nullptr; s.part = nullptr; s.nb = 0;
  int rc = dev_alloc((void **)&s.cnt, nb * sizeof(uint32_t), false);
  if (!rc) rc = dev_alloc((void **)&s.off, nb * sizeof(uint64_t), false);
  if (!rc) rc = dev_alloc((void **)&s.part, nb * LK_PART * sizeof(unsigned long long), false);
  if (rc) {
    hipFree(s.cnt); hipFree(s.off); hipFree(s.part);
    s.cnt = nullptr; s.off = nullptr; s.part = nullptr;
    return rc;
  }
  s.nb = nb;
  return 0;
}

// state image scratch: every array grows to what a call needs and is kept
void image_free(dint_engine *e) {
  hipFree(e->image.words); hipFree(e->image.blk); hipFree(e->image.blk_off); hipFree(e->image.inl); hipFree(e->image.ovf_src);
  e->image = dint_image_scratch{};
}
int image_alloc(dint_engine *e, uint32_t nb, uint64_t n_inl, uint64_t n_ovf) {
  dint_image_scratch &s = e->image;
  bool fresh = false;
  if (!s.words) {
    if (int rc = dev_alloc((void **)&s.words, DINT_IMAGE_WORDS * sizeof(unsigned long long))) return rc;
    fresh = true;
  }
  if (nb > s.nb || !s.blk) {
    hipFree(s.blk); hipFree(s.blk_off);
    s.blk = nullptr; s.blk_off = nullptr; s.nb = 0;
    int rc = dev_alloc((void **)&s.blk, (size_t)nb * sizeof(uint2));
    if (!rc) rc = dev_alloc((void **)&s.blk_off, (size_t)nb * sizeof(uint64_t));
    if (rc) return rc;
    s.nb = nb;
    fresh = true;
  }
  if (n_inl > s.n_inl) {
    hipFree(s.inl);
    s.inl = nullptr; s.n_inl = 0;
    if (int rc = dev_alloc((void **)&s.inl, (size_t)n_inl * sizeof(uint2), false)) return rc;
    s.n_inl = n_inl;
  }
  if (n_ovf > s.n_ovf) {
    hipFree(s.ovf_src);
    s.ovf_src = nullptr; s.n_ovf = 0;
    if (int rc = dev_alloc((void **)&s.ovf_src, (size_t)n_ovf * sizeof(uint32_t), false)) return rc;
    s.n_ovf = n_ovf;
  }
  if (fresh) HIP_TRY(hipDeviceSynchronize());  // (the zero fills ran on the null stream: the engine's stream does not wait for it)
  return 0;
}
// rehash scratch: every array grows to what a call needs and is kept
void rehash_free(dint_engine *e) {
  dint_rehash_scratch &s = e->rehash;
  hipFree(s.words); hipFree(s.blk); hipFree(s.blk_off); hipFree(s.key_in); hipFree(s.head); hipFree(s.loc_in); hipFree(s.key_out);
  hipFree(s.elist); hipFree(s.loc_out); hipFree(s.scan); hipFree(s.tmp); hipFree(s.src_entries);
  s = dint_rehash_scratch{};
}
int rehash_alloc(dint_engine *e, uint32_t nb, uint64_t n_max, uint64_t n_all, size_t tmp_bytes) {
  dint_rehash_scratch &s = e->rehash;
  bool fresh = false;
  if (!s.words) {
    int rc = dev_alloc((void **)&s.words, DINT_REHASH_WORDS * sizeof(unsigned long long));
    if (!rc) rc = dev_alloc((void **)&s.src_entries, (size_t)DINT_KV_MAX_TABLES * SR_MAX_SRCS * sizeof(uint8_t *));
    if (rc) return rc;
    fresh = true;
  }
  if (nb > s.nb || !s.blk) {
    hipFree(s.blk); hipFree(s.blk_off);
    s.blk = nullptr; s.blk_off = nullptr; s.nb = 0;
    int rc = dev_alloc((void **)&s.blk, (size_t)nb * sizeof(uint2));
    if (!rc) rc = dev_alloc((void **)&s.blk_off, (size_t)nb * sizeof(uint64_t));
    if (rc) return rc;
    s.nb = nb;
    fresh = true;
  }
  if (n_max > s.n_max) {
    hipFree(s.key_in); hipFree(s.head); hipFree(s.loc_in);
    s.key_in = s.head = nullptr; s.loc_in = nullptr; s.n_max = 0;
    int rc = dev_alloc((void **)&s.key_in, (size_t)n_max * sizeof(uint32_t), false);
    if (!rc) rc = dev_alloc((void **)&s.head, (size_t)n_max * sizeof(uint32_t), false);
    if (!rc) rc = dev_alloc((void **)&s.loc_in, (size_t)n_max * sizeof(uint64_t), false);
    if (rc) return rc;
    s.n_max = n_max;
  }
  if (n_all > s.n_all) {
    hipFree(s.key_out); hipFree(s.elist); hipFree(s.loc_out); hipFree(s.scan);
    s.key_out = s.elist = nullptr; s.loc_out = nullptr; s.scan = nullptr; s.n_all = 0;
    int rc = dev_alloc((void **)&s.key_out, (size_t)n_all * sizeof(uint32_t), false);
    if (!rc) rc = dev_alloc((void **)&s.elist, (size_t)n_all * sizeof(uint32_t), false);
    if (!rc) rc = dev_alloc((void **)&s.loc_out, (size_t)n_all * sizeof(uint64_t), false);
    if (!rc) rc = dev_alloc((void **)&s.scan, (size_t)(n_all + DINT_KV_MAX_TABLES) * sizeof(unsigned long long), false);
    if (rc) return rc;
    s.n_all = n_all;
  }
  if (tmp_bytes > s.tmp_bytes) {
    hipFree(s.tmp);
    s.tmp = nullptr; s.tmp_bytes = 0;
    if (int rc = dev_alloc(&s.tmp, tmp_bytes, false)) return rc;
    s.tmp_bytes = tmp_bytes;
  }
  if (fresh) HIP_TRY(hipDeviceSynchronize());  // (the zero fills ran on the null stream: the engine's stream does not wait for it)
  return 0;
}
// bulk load scratch: the arrays grow to what a call needs and are kept (dint_populate_device frees them when it is done)
void load_free(dint_engine *e) {
  dint_load_scratch &s = e->load;
  hipFree(s.words); hipFree(s.key_a); hipFree(s.idx_a); hipFree(s.key_b); hipFree(s.idx_b); hipFree(s.elist); hipFree(s.scan); hipFree(s.tmp);
  s = dint_load_scratch{};
}
size_t load_scratch_bytes(const dint_load_scratch &s) { return (size_t)s.n_max * 28 + 8 + s.tmp_bytes; }
int load_alloc(dint_engine *e, uint64_t n_max, size_t tmp_bytes) {
  dint_load_scratch &s = e->load;
  if (!s.words) {
    if (int rc = dev_alloc((void **)&s.words, DINT_LOAD_WORDS * sizeof(unsigned long long))) return rc;
    HIP_TRY(hipDeviceSynchronize());  // (the zero fill ran on the null stream: the engine's stream does not wait for it)
  }
  if (n_max > s.n_max) {
    hipFree(s.key_a); hipFree(s.idx_a); hipFree(s.key_b); hipFree(s.idx_b); hipFree(s.elist); hipFree(s.scan);
    s.key_a = s.idx_a = s.key_b = s.idx_b = s.elist = nullptr; s.scan = nullptr; s.n_max = 0;
    int rc = dev_alloc((void **)&s.key_a, (size_t)n_max * sizeof(uint32_t), false);
    if (!rc) rc = dev_alloc((void **)&s.idx_a, (size_t)n_max * sizeof(uint32_t), false);
    if (!rc) rc = dev_alloc((void **)&s.key_b, (size_t)n_max * sizeof(uint32_t), false);
    if (!rc) rc = dev_alloc((void **)&s.idx_b, (size_t)n_max * sizeof(uint32_t), false);
    if (!rc) rc = dev_alloc((void **)&s.elist, (size_t)n_max * sizeof(uint32_t), false);
    if (!rc) rc = dev_alloc((void **)&s.scan, (size_t)(n_max + 1) * sizeof(unsigned long long), false);
    if (rc) return rc;
    s.n_max = n_max;
  }
  if (tmp_bytes > s.tmp_bytes) {
    hipFree(s.tmp);
    s.tmp = nullptr; s.tmp_bytes = 0;
    if (int rc = dev_alloc(&s.tmp, tmp_bytes, false)) return rc;
    s.tmp_bytes = tmp_bytes;
  }
  return 0;
}
// the layout-relevant flags an image carries
uint32_t image_flags(const dint_engine *e) { return e->cfg.workload == DINT_WL_TATP ? (e->cfg.flags & DINT_FLAG_LOCK_SAME_KEY) : 0u; }

// the records appended since the last drain, oldest first, to host (dint_log_drain) or device memory (dint_log_drain_device):
// one cursor, one contract
int64_t log_drain_locked(dint_engine *e, void *records, uint64_t cap, uint64_t *lost, bool to_device, hipStream_t st) {
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  uint32_t t[4];
  HIP_TRY(hipMemcpy(t, e->log.tail, sizeof t, hipMemcpyDeviceToHost));
  LgRing r = {{t[0], t[1]}, (uint64_t)t[2] | ((uint64_t)t[3] << 32), e->log_drained, e->log_gone};
  const LgDrain d = lg_drain(r, e->log.cap, cap);  // (log_ring.h: the cursor, what the ring lapped, where the records start)
  if (lost) *lost = d.lost;
  const uint64_t n = d.n;
  uint64_t pos = d.pos;  // record k of the stream lives at ring slot k % cap
  uint8_t *out = (uint8_t *)records;
  for (uint64_t done = 0; done < n;) {
    const uint64_t run = std::min<uint64_t>(n - done, e->log.cap - pos);
    if (to_device) HIP_TRY(hipMemcpyAsync(out + done * 64, e->log.ring + pos * 64, run * 64, hipMemcpyDeviceToDevice, st));
    else HIP_TRY(hipMemcpy(out + done * 64, e->log.ring + pos * 64, run * 64, hipMemcpyDeviceToHost));
    done += run;
    pos = (pos + run) % e->log.cap;
  }
  if (to_device && n) HIP_TRY(hipStreamSynchronize(st));  // the records are complete when the call returns
  e->log_drained = r.drained; e->log_gone = r.gone;
  return (int64_t)n;
}

}  // namespace

void dint_set_last_error(const char *msg) { g_err = msg ? msg : ""; }

extern "C" {

const char *dint_last_error(void) { return g_err.c_str(); }

int dint_msg_size(uint32_t workload) { return workload < DINT_WL_COUNT ? kMsgSize[workload] : DINT_EINVAL; }

int dint_engine_create(const dint_config *cfg, dint_engine_t **out) {
  if (!cfg || !out) return fail(DINT_EINVAL, "null argument");
  if (cfg->abi_version != DINT_ABI_VERSION) return fail(DINT_EINVAL, "abi_version %u != %u", cfg->abi_version, DINT_ABI_VERSION);
  if (cfg->workload >= DINT_WL_COUNT) return fail(DINT_EINVAL, "unknown workload %u", cfg->workload);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(DINT_ENODEV, "no HIP device");
  int dev = cfg->device;
  if (dev < 0) HIP_TRY(hipGetDevice(&dev));
  if (dev >= ndev) return fail(DINT_ENODEV, "device %d of %d", dev, ndev);
  HIP_TRY(hipSetDevice(dev));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, dev));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(DINT_ENODEV, "device %d is %s, this library is built for gfx950 only", dev, prop.gcnArchName);

  dint_engine *e = new dint_engine();
  e->cfg = *cfg;
  e->device = dev;
  e->msg_size = kMsgSize[cfg->workload];
  e->shard.count = cfg->shard_count ? cfg->shard_count : 1;
  e->shard.index = cfg->shard_index;
  int rc = 0;
#define TRY(x) do { rc = (x); if (rc) { dint_engine_destroy(e); return rc; } } while (0)
  if (e->shard.index >= e->shard.count || e->shard.count > 255) {
    delete e;
    return fail(DINT_EINVAL, "shard %u of %u", cfg->shard_index, cfg->shard_count);
  }
  // (the copy streams of the host path exist only with DINT_FLAG_COPY_STREAMS, and are created on first use)
  // (a high-priority engine stream beside the wide routing kernels of a sharded step was measured: --force-exchange 1,310 ->
  // 804 Mtxn/s; DINT_ENGINE_PRIORITY keeps the knob)
  const char *pe = getenv("DINT_ENGINE_PRIORITY");
  const int prio = pe ? atoi(pe) : 0;
  if (hipStreamCreateWithPriority(&e->stream, hipStreamNonBlocking, prio) != hipSuccess ||
      hipEventCreateWithFlags(&e->ev_order, hipEventDisableTiming) != hipSuccess) {
    dint_engine_destroy(e);
    return fail(DINT_EHIP, "hipStreamCreate");
  }
  const uint32_t wl = cfg->workload;
  const bool is_kv = wl == DINT_WL_STORE || wl == DINT_WL_TATP || wl == DINT_WL_SMALLBANK;
  // requests per kernel pass: the request index must fit the batch record (20 bits)
  // The lock tables default to BASELINE's batch size: their dominant-slot path (index bitmaps, k_locks.hip) covers passes of
  // up to 65,536 requests, and a longer pass runs 3x (lock_fasst) to 16x (lock_2pl) slower PER REQUEST on a Zipf stream (r05
  // bench, pass_1m) -- so a dint_submit of a million requests is sixteen passes unless the caller asks for longer ones.
  e->pass_max = (wl == DINT_WL_FASST || wl == DINT_WL_2PL) ? DINT_MICRO_BATCH : DINT_KV_PASS;
  if (cfg->max_pass) e->pass_max = std::min<uint32_t>(DINT_KV_PASS, std::max<uint32_t>(cfg->max_pass, 64u));
  if (wl == DINT_WL_LOG || wl == DINT_WL_TATP || wl == DINT_WL_SMALLBANK) {
    // a pass never laps the log ring, so a DELETE_LOG record keeps the val bytes of the record it overwrites
    // exactly as in the serial reference
    const uint32_t cap = cfg->log_entries ? cfg->log_entries : 1000000u;
    e->pass_max = std::min<uint32_t>(e->pass_max, cap);
  }
  TRY(dev_alloc((void **)&e->scratch.stats, sizeof(dint_dev_stats)));
  add_region(e, e->scratch.stats, sizeof(dint_dev_stats));
  if (wl != DINT_WL_LOG) {  // the bins of one pass: 64 records in place per bin + the pass's overflow area
    TRY(dev_alloc((void **)&e->scratch.bin_cnt, DINT_KV_PMAX * sizeof(uint32_t)));
    if (is_kv) {
      // coarse bins of 16-byte records, DINT_KV_CAP_MULT (64) times the mean load in place each: C * cap = C * (64 ceil(n / C)
      // + 64) <= 64 n + 128 C slots -- 1 GB for passes of 2^20 requests, of which a pass touches what it fills.  (r04 / r05
      // kept 2 x the mean and sent a hot key's excess to the pass's overflow list, which every bin that has records there
      // reads from end to end, twice: smallbank at Zipf 0.99 -- 100,000 entries, a dozen such bins -- spent 100 us of its
      // 135 us resolve kernel there.  288 GB of HBM are there to be used.)
      e->scratch.kbins_slots = (uint64_t)dint_kv_cap_mult() * e->pass_max + 128ull * DINT_KV_CMAX;
      TRY(dev_alloc((void **)&e->scratch.kbins, (size_t)e->scratch.kbins_slots * sizeof(uint4), false));
      TRY(dev_alloc((void **)&e->scratch.bigq, (size_t)DINT_KV_BIGQ_MAX * 3 * sizeof(uint4), false));  // KVQ_W uint4 per work item (k_kv.hip)
      TRY(dev_alloc((void **)&e->scratch.hotpub, (size_t)DINT_KV_HOTPUB_WORDS * sizeof(unsigned long long)));
      TRY(dev_alloc((void **)&e->scratch.lateq, (size_t)DINT_KV_BIGQ_MAX * sizeof(uint4), false));
      // the second set of what the partition stage writes (dint_kv_sets): 288 GB of HBM are there to be used
      TRY(dev_alloc((void **)&e->scratch.kvs.bin_cnt[1], DINT_KV_PMAX * sizeof(uint32_t)));
      TRY(dev_alloc((void **)&e->scratch.kvs.kbins[1], (size_t)e->scratch.kbins_slots * sizeof(uint4), false));
      TRY(dev_alloc((void **)&e->scratch.kvs.ovl[1], (size_t)e->pass_max * sizeof(uint4) * 2, false));
      TRY(dev_alloc((void **)&e->scratch.kvs.bigrdy, (size_t)DINT_KV_BIGQ_MAX * sizeof(uint32_t)));
      if (wl == DINT_WL_SMALLBANK)  // what the pieces of a hot account's row tell each other: 40 words per work item (kv_sb_item)
        TRY(dev_alloc((void **)&e->scratch.kvs.sbx, (size_t)DINT_KV_BIGQ_MAX * DINT_KV_SBX_WORDS * sizeof(uint64_t), false));
    } else {
      TRY(dev_alloc((void **)&e->scratch.bins, (size_t)DINT_KV_PMAX * DINT_KV_BINCAP * sizeof(uint64_t), false));
      // lock tables, passes of <= 65,536 requests (k_locks.hip, LK_DIRECT_NMAX): a big bin's records beyond the 64 in place go
      // straight to a region of its own -- 1,024 regions (a pass of 65,536 has at most that many bins of more than 64) of
      // 65,536 records (a bin holds at most the pass): 512 MB of address space, touched as filled.  DINT_LOCK_NO_DIRECT at
      // creation: not allocated (r01-r05's overflow list + k_kv_scan_place for every pass).
      if (!getenv("DINT_LOCK_NO_DIRECT")) {
        e->scratch.kbins_slots = 1024ull * 65536ull;
        TRY(dev_alloc((void **)&e->scratch.kbins, (size_t)e->scratch.kbins_slots * sizeof(uint64_t), false));
      }
    }
    TRY(dev_alloc((void **)&e->scratch.blk_pub, 3 * 1024 * sizeof(uint32_t)));
    e->scratch.blk_pub_next = e->scratch.blk_pub + 1024;
    TRY(dev_alloc((void **)&e->scratch.big, 2 * (4 + DINT_KV_PMAX) * sizeof(uint32_t)));
    e->scratch.big_next = e->scratch.big + (4 + DINT_KV_PMAX);
    if (is_kv)  // (the three sets of control words and tile counts live in the allocations the lock tables use as two)
      for (int k = 0; k < 3; k++) { e->scratch.kvs.ctl[k] = e->scratch.big + DINT_KV_CTL_WORDS * k; e->scratch.kvs.pub[k] = e->scratch.blk_pub + 1024 * k; }
    TRY(dev_alloc((void **)&e->scratch.bin_off, DINT_KV_PMAX * sizeof(uint32_t)));
    TRY(hipMemset(e->scratch.bin_off, 0xFF, DINT_KV_PMAX * sizeof(uint32_t)) == hipSuccess ? 0 : fail(DINT_EHIP, "hipMemset"));  // (lock tables, direct big bins: "no region named" between passes)
    TRY(dev_alloc((void **)&e->scratch.ovl, (size_t)e->pass_max * sizeof(uint4) * (is_kv ? 2 : 1), false));
    TRY(dev_alloc((void **)&e->scratch.ovf, (size_t)e->pass_max * sizeof(uint64_t), false));
    if (is_kv) {
      TRY(dev_alloc((void **)&e->scratch.ovf2, (size_t)e->pass_max * sizeof(uint64_t), false));
      e->scratch.kvs.bin_cnt[0] = e->scratch.bin_cnt; e->scratch.kvs.kbins[0] = e->scratch.kbins; e->scratch.kvs.ovl[0] = e->scratch.ovl;
    }
    if ((e->cfg.workload == DINT_WL_FASST || e->cfg.workload == DINT_WL_2PL) && getenv("DINT_KV_TRACE")) {
      TRY(dev_alloc((void **)&e->kv.d_trace, (size_t)DINT_KV_TRACE_WORDS * 8, true));
      e->scratch.lock_trace = e->kv.d_trace;
    }
  } else {  // the log append has no bins: per-block counts of its scan only
    TRY(dev_alloc((void **)&e->scratch.blk_pub, 2 * (1024 + 16) * sizeof(uint32_t)));  // per tile: valid requests; + ticket, finished
    e->scratch.blk_pub_next = e->scratch.blk_pub + (1024 + 16);
  }
  TRY(slot_alloc(e, 0));
  if (hipHostMalloc((void **)&e->h_pinned, (size_t)e->pass_max * e->msg_size + 64, hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc((void **)&e->h_pool, 64, hipHostMallocDefault) != hipSuccess) {
    dint_engine_destroy(e);
    return fail(DINT_ENOMEM, "hipHostMalloc");
  }
  e->h_pool[0] = e->h_pool[1] = 0;  // [0] read back with each host chunk (dint_wait), [1] by dint_sync

  if (wl == DINT_WL_FASST || wl == DINT_WL_2PL) {
    e->n_slots = cfg->n_slots ? cfg->n_slots : 36000000ull;  // lock_fasst/udp/utils.h:12
    if (e->n_slots > 0xFFFFFFF0ull) { dint_engine_destroy(e); return fail(DINT_EINVAL, "n_slots too large"); }
    e->slots_mod = dint_make_mod(e->n_slots);
    e->n_local_slots = (e->n_slots + e->shard.count - 1) / e->shard.count;
    TRY(dev_alloc((void **)&e->d_lock_tbl, e->n_local_slots * sizeof(uint2)));
    add_region(e, e->d_lock_tbl, e->n_local_slots * sizeof(uint2));
  }
  if (wl == DINT_WL_LOG || wl == DINT_WL_TATP || wl == DINT_WL_SMALLBANK) {
    e->log.cap = cfg->log_entries ? cfg->log_entries : 1000000u;  // log_server/udp/utils.h:16
    TRY(dev_alloc((void **)&e->log.ring, (size_t)e->log.cap * 64));
    TRY(dev_alloc((void **)&e->log.tail, 4 * sizeof(uint32_t)));
    add_region(e, e->log.ring, (size_t)e->log.cap * 64);
    add_region(e, e->log.tail, 4 * sizeof(uint32_t));
  }
  if (is_kv) {
    rc = dint_kv_create(&e->kv, wl, cfg->n_rows, e->shard, cfg->pool_entries, cfg->flags);
    if (rc) { dint_engine_destroy(e); return fail(rc, "kv table allocation failed (%s)", g_err.c_str()); }
    // the owner-key comparison of DINT_FLAG_LOCK_SAME_KEY exists on the request-by-request path only
    e->kv.force_rounds = ((cfg->flags & (DINT_FLAG_KV_ROUNDS | DINT_FLAG_LOCK_SAME_KEY)) ? 1 : 0) |
                         ((cfg->flags & DINT_FLAG_KV_NO_HOT) ? 2 : 0);
    for (auto &r : dint_kv_regions(&e->kv)) add_region(e, r.first, r.second);
  }
  if (hipDeviceSynchronize() != hipSuccess) {
    dint_engine_destroy(e);
    return fail(DINT_EHIP, "hipDeviceSynchronize after engine set-up");
  }
#undef TRY
  *out = e;
  return 0;
}

void dint_engine_destroy(dint_engine_t *e) {
  if (!e) return;
  hipSetDevice(e->device);
  hipDeviceSynchronize();
  for (auto &sl : e->slot)  // (everything has left the GPU: undelivered replies of pageable callers are not dropped)
    if (sl.deliver_to && sl.h_rep) { memcpy(sl.deliver_to, sl.h_rep, sl.deliver_bytes); sl.deliver_to = nullptr; }
  for (hipEvent_t ev : e->timer.ev) hipEventDestroy(ev);
  for (void *p : e->snap) hipFree(p);
  hipFree(e->scratch.bin_cnt);
  hipFree(e->scratch.bins);
  hipFree(e->scratch.kbins);
  hipFree(e->scratch.bigq);
  hipFree(e->scratch.hotpub);
  hipFree(e->scratch.lateq);
  hipFree(e->scratch.kvs.bin_cnt[1]);
  hipFree(e->scratch.kvs.kbins[1]);
  hipFree(e->scratch.kvs.ovl[1]);
  hipFree(e->scratch.kvs.bigrdy);
  hipFree(e->scratch.kvs.sbx);
  hipFree(e->scratch.stats);
  hipFree(e->scratch.blk_cnt);
  hipFree(std::min(e->scratch.blk_pub, e->scratch.blk_pub_next));
  hipFree(std::min(e->scratch.big, e->scratch.big_next));
  hipFree(e->scratch.bin_off);
  hipFree(e->scratch.ovl);
  hipFree(e->scratch.ovf);
  hipFree(e->scratch.ovf2);
  if (e->scratch.lock_trace) { hipFree(e->scratch.lock_trace); e->kv.d_trace = nullptr; }
  for (auto &sl : e->slot) {
    hipFree(sl.d_req);
    hipFree(sl.d_rep);
    if (sl.h_req) hipHostFree(sl.h_req);
    if (sl.h_rep) hipHostFree(sl.h_rep);
    if (sl.h2d) hipEventDestroy(sl.h2d);
    if (sl.comp) hipEventDestroy(sl.comp);
    if (sl.done) hipEventDestroy(sl.done);
  }
  hipFree(std::min(e->route.blk, e->route.blk_next));
  if (e->h_pinned) hipHostFree(e->h_pinned);
  if (e->h_pool) hipHostFree(e->h_pool);
  if (e->ev_order) hipEventDestroy(e->ev_order);
  if (e->ev_route_order) hipEventDestroy(e->ev_route_order);
  if (e->ev_wait) hipEventDestroy(e->ev_wait);
  if (e->ev_signal) hipEventDestroy(e->ev_signal);
  if (e->s_h2d && e->s_h2d != e->stream) hipStreamDestroy(e->s_h2d);
  if (e->s_d2h && e->s_d2h != e->stream) hipStreamDestroy(e->s_d2h);
  lock_pipe_destroy(e);
  replay_free(e);
  fold_free(e);
  state_free(e);
  block_free(e);
  rroute_free(e);
  hipFree(e->tstats.part); hipFree(e->tstats.out);
  e->tstats = dint_stats_scratch{};
  locks_free(e);
  dint_verify_free(e->tverify);
  dint_compact_free(e->tcompact);
  image_free(e);
  rehash_free(e);
  load_free(e);
  for (hipEvent_t ev : e->ev_load)
    if (ev) hipEventDestroy(ev);
  for (hipEvent_t ev : e->ev_replay)
    if (ev) hipEventDestroy(ev);
  for (hipEvent_t ev : e->ev_fold)
    if (ev) hipEventDestroy(ev);
  for (hipEvent_t ev : e->ev_rehash)
    if (ev) hipEventDestroy(ev);
  for (hipEvent_t ev : e->ev_verify)
    if (ev) hipEventDestroy(ev);
  for (hipEvent_t ev : e->ev_compact)
    if (ev) hipEventDestroy(ev);
  hipFree(e->d_lock_tbl);
  hipFree(e->log.ring);
  hipFree(e->log.tail);
  dint_kv_destroy(&e->kv);
  if (e->stream) hipStreamDestroy(e->stream);
  delete e;
}

namespace {
int submit_device_locked(dint_engine *e, const void *d_reqs, uint32_t n, void *d_replies, const void *d_next_reqs, uint32_t next_n,
                         void *d_next_replies, void *stream) {
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t st = stream ? (hipStream_t)stream : e->stream;
  const uint8_t *rq = (const uint8_t *)d_reqs;
  uint8_t *rp = (uint8_t *)d_replies;
  if (int rc = ahead_settle(e)) return rc;
  if (n == 0 && e->ahead.valid) return run_pass(e, d_reqs, 0, d_replies, st);  // (reports the broken announcement)
  for (uint32_t off = 0; off < n; off += e->pass_max) {
    uint32_t m = std::min<uint32_t>(e->pass_max, n - off);
    // what the engine's next pass will be: the next slice of this array (stream order has it complete: the whole array
    // precedes this call) -- or the first pass of the batch the caller announced
    dint_kv_ahead nx = {nullptr, nullptr, 0, dint_flat_view()};
    if (off + m < n) {
      nx.d_req = rq + (size_t)(off + m) * e->msg_size; nx.d_rep = rp + (size_t)(off + m) * e->msg_size;
      nx.n = std::min<uint32_t>(e->pass_max, n - off - m);
    } else if (next_n) {
      nx.d_req = d_next_reqs; nx.d_rep = d_next_replies; nx.n = std::min<uint32_t>(e->pass_max, next_n);
    }
    int rc = run_pass(e, rq + (size_t)off * e->msg_size, m, rp + (size_t)off * e->msg_size, st, 0, dint_flat_view(),
                      (e->cfg.flags & DINT_FLAG_INPUTS_READY) != 0,
                      (e->kv.n_tables || e->cfg.workload == DINT_WL_FASST || e->cfg.workload == DINT_WL_2PL) && nx.n ? &nx : nullptr);
    if (rc) return rc;
  }
  return 0;
}
}  // namespace

int dint_submit_device(dint_engine_t *e, const void *d_reqs, uint32_t n, void *d_replies, void *stream) {
  if (!e || (n && (!d_reqs || !d_replies))) return fail(DINT_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  return submit_device_locked(e, d_reqs, n, d_replies, nullptr, 0, nullptr, stream);
}

int dint_submit_device_ahead(dint_engine_t *e, const void *d_reqs, uint32_t n, void *d_replies, const void *d_next_reqs,
                             uint32_t next_n, void *d_next_replies, void *stream) {
  if (!e || (n && (!d_reqs || !d_replies)) || (next_n && (!d_next_reqs || !d_next_replies))) return fail(DINT_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  return submit_device_locked(e, d_reqs, n, d_replies, d_next_reqs, next_n, d_next_replies, stream);
}

int dint_submit_segments(dint_engine_t *e, void *d_base, uint32_t n_seg, uint32_t seg_cap, uint64_t seg_stride,
                         const void *d_cnt, uint64_t cnt_stride, void *stream) {
  if (!e || (n_seg && (!d_base || !d_cnt))) return fail(DINT_EINVAL, "null argument");
  if (seg_cap < 2 || seg_cap > e->pass_max) return fail(DINT_EINVAL, "seg_cap %u outside [2, %u]", seg_cap, e->pass_max);
  if (seg_stride < (uint64_t)seg_cap * e->msg_size) return fail(DINT_EINVAL, "seg_stride smaller than a segment");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t st = stream ? (hipStream_t)stream : e->stream;
  const uint32_t per_pass = e->pass_max / seg_cap;  // whole segments per kernel pass
  for (uint32_t k0 = 0; k0 < n_seg; k0 += per_pass) {
    const uint32_t ns = std::min(per_pass, n_seg - k0);
    uint8_t *base = (uint8_t *)d_base + (size_t)k0 * seg_stride;
    const dint_view v = dint_seg_view(ns, seg_cap, seg_stride, (const uint8_t *)d_cnt + (size_t)k0 * cnt_stride, cnt_stride);
    int rc = run_pass(e, base, ns * seg_cap, base, st, 0, v);
    if (rc) return rc;
  }
  return 0;
}

int dint_submit_segments_multi(const dint_segments_item *items, uint32_t n_items, void *stream) {
  return dint_submit_segments_multi_ahead(items, n_items, nullptr, stream);
}

int dint_submit_segments_multi_ahead(const dint_segments_item *items, uint32_t n_items, const dint_segments_item *next, void *stream) {
  if (!items || n_items == 0) return fail(DINT_EINVAL, "null argument");
  for (uint32_t k = 0; k < n_items; k++) {
    if (!items[k].engine) return fail(DINT_EINVAL, "null engine");
    for (uint32_t j = 0; j < k; j++)
      if (items[j].engine == items[k].engine) return fail(DINT_EINVAL, "an engine appears twice");
  }
  hipStream_t st = stream ? (hipStream_t)stream : items[0].engine->stream;
  bool one_set = n_items <= DINT_KV_MULTI_MAX;
  for (uint32_t k = 0; k < n_items && one_set; k++) {
    const dint_engine *e = items[k].engine;
    const uint32_t wl = e->cfg.workload;
    one_set = (wl == DINT_WL_STORE || wl == DINT_WL_TATP || wl == DINT_WL_SMALLBANK) && wl == items[0].engine->cfg.workload &&
              e->device == items[0].engine->device && items[k].n_seg > 0 && items[k].seg_cap >= 2 &&
              (uint64_t)items[k].n_seg * items[k].seg_cap <= e->pass_max &&
              // (the launch takes `hot` and the workers from the first engine: all must resolve hot keys the same way)
              !((e->cfg.flags ^ items[0].engine->cfg.flags) & (DINT_FLAG_KV_ROUNDS | DINT_FLAG_KV_NO_HOT | DINT_FLAG_LOCK_SAME_KEY));
  }
  if (!one_set) {
    for (uint32_t k = 0; k < n_items; k++)
      if (int rc = dint_submit_segments(items[k].engine, items[k].d_base, items[k].n_seg, items[k].seg_cap, items[k].seg_stride,
                                        items[k].d_cnt, items[k].cnt_stride, st))
        return rc;
    return 0;  // (an announcement is dropped: nothing ran ahead)
  }
  // the announced next step: the same engines, the same geometry, other buffers -- else it is ignored
  for (uint32_t k = 0; next && k < n_items; k++)
    if (next[k].engine != items[k].engine || !next[k].d_base || !next[k].d_cnt || next[k].n_seg != items[k].n_seg ||
        next[k].seg_cap != items[k].seg_cap || next[k].seg_stride != items[k].seg_stride || next[k].cnt_stride != items[k].cnt_stride)
      next = nullptr;
  if (next && !dint_kv_multi_ahead_ok(items[0].engine->kv)) next = nullptr;
  // every argument is checked before an engine is locked or a stream ordered: an EINVAL on item k must not leave the
  // engines of items 0 .. k-1 with a new last_stream and a stale ordering event
  for (uint32_t k = 0; k < n_items; k++) {
    const dint_segments_item &it = items[k];
    if (!it.d_base || !it.d_cnt) return fail(DINT_EINVAL, "null argument");
    if (it.seg_stride < (uint64_t)it.seg_cap * it.engine->msg_size) return fail(DINT_EINVAL, "seg_stride smaller than a segment");
  }
  std::vector<dint_engine *> es;
  for (uint32_t k = 0; k < n_items; k++) es.push_back(items[k].engine);
  std::sort(es.begin(), es.end());
  std::vector<std::unique_lock<std::mutex>> locks;
  for (dint_engine *e : es) locks.emplace_back(e->mu);  // address order: two calls that share engines cannot deadlock
  HIP_TRY(hipSetDevice(items[0].engine->device));
  dint_kv_pass pass[DINT_KV_MULTI_MAX], npass[DINT_KV_MULTI_MAX];
  // what ran ahead: all of the engines' partitions (the previous call of this kind announced exactly this step), or none
  uint32_t n_done = 0;
  for (uint32_t k = 0; k < n_items; k++) {
    if (int rc = ahead_settle(items[k].engine)) return rc;
    const dint_engine::Ahead &a = items[k].engine->ahead;
    if (a.valid && a.req == items[k].d_base && a.n == items[k].n_seg * items[k].seg_cap && a.seg_cap == items[k].seg_cap &&
        a.n_seg == items[k].n_seg && a.cnt == items[k].d_cnt)
      n_done++;
    else if (a.valid)
      n_done = 0xFFFFu;
  }
  if (n_done != 0 && n_done != n_items) {
    for (uint32_t k = 0; k < n_items; k++)
      if (int rc = ahead_cancel(items[k].engine)) return rc;
    return fail(DINT_ESTATE, "a batch announced by dint_submit_device_ahead / dint_submit_segments_multi_ahead must be the engine's next submission");
  }
  const bool part_done = n_done == n_items;
  for (uint32_t k = 0; k < n_items; k++) {
    items[k].engine->ahead.valid = false;
    items[k].engine->ahead.broken.reset();
  }
  std::shared_ptr<std::atomic<bool>> set_word;
  if (next) set_word = std::make_shared<std::atomic<bool>>(false);
  for (uint32_t k = 0; k < n_items; k++) {
    const dint_segments_item &it = items[k];
    dint_engine *e = it.engine;
    e->blank = false, e->fresh = 0;
    if (int rc = order_stream(e, st)) return rc;
    if (int rc = next_pass_seq(e, st)) return rc;
    pass[k].d_req = it.d_base; pass[k].d_rep = it.d_base; pass[k].n = it.n_seg * it.seg_cap;
    pass[k].kv = &e->kv; pass[k].log = e->log; pass[k].s = e->scratch;
    pass[k].view = dint_seg_view(it.n_seg, it.seg_cap, it.seg_stride, it.d_cnt, it.cnt_stride);
    if (next) {
      npass[k] = pass[k];
      npass[k].d_req = next[k].d_base; npass[k].d_rep = next[k].d_base;
      npass[k].view = dint_seg_view(it.n_seg, it.seg_cap, it.seg_stride, next[k].d_cnt, it.cnt_stride);
    }
  }
  dint_launch_kv_multi(pass, n_items, st, part_done, next ? npass : nullptr);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(DINT_EHIP, "kernel launch: %s", hipGetErrorString(err));
  for (uint32_t k = 0; k < n_items; k++) {
    dint_engine *e = items[k].engine;
    if (int rc = mark_stream(e, st)) return rc;
    e->batches++;
    e->requests += pass[k].n;
    if (next) {
      e->ahead.valid = true;
      e->ahead.req = next[k].d_base; e->ahead.rep = next[k].d_base; e->ahead.n = pass[k].n;
      e->ahead.seg_cap = items[k].seg_cap; e->ahead.n_seg = items[k].n_seg; e->ahead.cnt = next[k].d_cnt;
      e->ahead.broken = set_word;
    }
  }
  return 0;
}

// ---- host buffers: pipelined H2D / kernels / D2H ---------------------------------------------------------------
namespace {
// enqueue chunk [off, off + m) of a host submission; returns its sequence number in *seq
// is [p, p + bytes) page-locked memory the HIP runtime knows (dint_alloc_pinned, hipHostMalloc, hipHostRegister)?
bool host_range_pinned(const void *p, size_t bytes) {
  if (bytes == 0) return true;
  static const bool no_bounce = getenv("DINT_NO_BOUNCE") != nullptr;  // diagnostic (tools/stress_pageable.py): r04's direct copies
  if (no_bounce) return true;
  const uint8_t *ends[2] = {(const uint8_t *)p, (const uint8_t *)p + bytes - 1};
  for (const uint8_t *q : ends) {
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof a);
    if (hipPointerGetAttributes(&a, q) != hipSuccess) {
      (void)hipGetLastError();  // an unregistered pointer is an error to older runtimes: not ours
      return false;
    }
    if (a.type != hipMemoryTypeHost) return false;  // hipMemoryTypeUnregistered (plain memory), or not host memory at all
  }
  return true;
}
// a DEVICE pointer handed to the host path (dint_submit / dint_submit_async): the staging memcpy would read it on the CPU
bool is_device_ptr(const void *p) {
  if (!p) return false;
  hipPointerAttribute_t a;
  memset(&a, 0, sizeof a);
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.type == hipMemoryTypeDevice;
}
// copy a delivered chunk's replies out of the slot's bounce buffer (the chunk has left the GPU: sl.done was waited for)
void slot_deliver(dint_engine::Slot &sl) {
  if (sl.deliver_to) memcpy(sl.deliver_to, sl.h_rep, sl.deliver_bytes);
  sl.deliver_to = nullptr;
  sl.deliver_bytes = 0;
}
int slot_bounce_alloc(dint_engine *e, dint_engine::Slot &sl, bool req, bool rep) {
  const size_t bytes = (size_t)e->pass_max * e->msg_size + 64;
  if (req && !sl.h_req && hipHostMalloc((void **)&sl.h_req, bytes, hipHostMallocDefault) != hipSuccess)
    return fail(DINT_ENOMEM, "hipHostMalloc(%zu) for the staging of a pageable request buffer", bytes);
  if (rep && !sl.h_rep && hipHostMalloc((void **)&sl.h_rep, bytes, hipHostMallocDefault) != hipSuccess)
    return fail(DINT_ENOMEM, "hipHostMalloc(%zu) for the staging of a pageable reply buffer", bytes);
  return 0;
}
int enqueue_chunk(dint_engine *e, const uint8_t *rq, uint8_t *rp, uint32_t m, uint64_t *seq, bool rq_pinned, bool rp_pinned) {
  const uint64_t sq = e->next_seq;
  const int k = (int)(sq % dint_engine::kNSlot);
  if (int rc = slot_alloc(e, k)) return rc;
  if (!e->s_h2d) {
    if (!(e->cfg.flags & DINT_FLAG_COPY_STREAMS)) {
      // default: copies on the engine's own stream.  Measured on MI355X (same-box A/B, r02; NOTEBOOK.md): with three engines
      // in one process, two more streams per engine push the process past HIP's 4 hardware queues and -- depending on
      // which queues end up shared -- serialise the engines' kernel chains (TATP replay 1.2 instead of 1.7 G txn/s).
      // Several engines overlap each other's copies anyway; one engine alone wants DINT_FLAG_COPY_STREAMS.
      e->s_h2d = e->s_d2h = e->stream;
    } else {
      HIP_TRY(hipStreamCreateWithFlags(&e->s_h2d, hipStreamNonBlocking));
      HIP_TRY(hipStreamCreateWithFlags(&e->s_d2h, hipStreamNonBlocking));
    }
  }
  dint_engine::Slot &sl = e->slot[k];
  if (sl.seq) HIP_TRY(hipEventSynchronize(sl.done));  // the slot's previous chunk has left the GPU
  slot_deliver(sl);                                    // ... and, for a pageable caller, reaches its reply buffer now
  const size_t bytes = (size_t)m * e->msg_size;
  if (int rc = slot_bounce_alloc(e, sl, !rq_pinned, !rp_pinned)) return rc;
  if (!rq_pinned) {
    memcpy(sl.h_req, rq, bytes);
    rq = sl.h_req;
  }
  HIP_TRY(hipMemcpyAsync(sl.d_req, rq, bytes, hipMemcpyHostToDevice, e->s_h2d));
  HIP_TRY(hipEventRecord(sl.h2d, e->s_h2d));
  HIP_TRY(hipStreamWaitEvent(e->stream, sl.h2d, 0));
  if (int rc = run_pass(e, sl.d_req, m, sl.d_rep, e->stream)) return rc;
  HIP_TRY(hipEventRecord(sl.comp, e->stream));
  HIP_TRY(hipStreamWaitEvent(e->s_d2h, sl.comp, 0));
  if (!rp_pinned) {
    sl.deliver_to = rp;
    sl.deliver_bytes = bytes;
    rp = sl.h_rep;
  }
  HIP_TRY(hipMemcpyAsync(rp, sl.d_rep, bytes, hipMemcpyDeviceToHost, e->s_d2h));
  if (e->kv.n_tables)  // the overflow-pool counter travels with the replies (see dint_wait)
    HIP_TRY(hipMemcpyAsync(e->h_pool, &e->scratch.stats->pool_exhausted, sizeof(unsigned long long), hipMemcpyDeviceToHost, e->s_d2h));
  HIP_TRY(hipEventRecord(sl.done, e->s_d2h));
  sl.seq = sq;
  e->next_seq++;
  *seq = sq;
  return 0;
}
int wait_seq(dint_engine *e, uint64_t seq) {
  if (seq == 0 || seq >= e->next_seq) return fail(DINT_EINVAL, "unknown ticket");
  dint_engine::Slot &sl = e->slot[seq % dint_engine::kNSlot];
  if (sl.seq == seq) HIP_TRY(hipEventSynchronize(sl.done));  // else: the slot was reused, so the chunk finished long ago
  // replies of `seq` and of every earlier chunk are complete: the ones that went through a bounce buffer reach the
  // caller's memory here (chunks are enqueued, and leave the GPU, in sequence order)
  for (auto &o : e->slot)
    if (o.deliver_to && o.seq <= seq) {
      if (o.seq != seq) HIP_TRY(hipEventSynchronize(o.done));
      slot_deliver(o);
    }
  if (*e->h_pool > e->pool_seen) {
    const unsigned long long lost = *e->h_pool - e->pool_seen;
    e->pool_seen = *e->h_pool;
    return fail(DINT_ENOMEM, "%llu INSERTs found the overflow-entry pool full (dint_config.pool_entries); "
                             "they were answered with a reject code and stored nothing", lost);
  }
  return 0;
}
}  // namespace

int dint_submit_async(dint_engine_t *e, const void *reqs, uint32_t n, void *replies, dint_ticket *ticket) {
  if (!e || !ticket || (n && (!reqs || !replies))) return fail(DINT_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->device));
  const uint8_t *rq = (const uint8_t *)reqs;
  uint8_t *rp = (uint8_t *)replies;
  uint64_t seq = e->next_seq - 1;  // n == 0: the ticket of whatever was submitted last
  if (n && (is_device_ptr(rq) || is_device_ptr(rp)))
    return fail(DINT_EINVAL, "dint_submit / dint_submit_async take HOST buffers; device memory goes to dint_submit_device");
  const bool rq_pinned = host_range_pinned(rq, (size_t)n * e->msg_size), rp_pinned = host_range_pinned(rp, (size_t)n * e->msg_size);
  for (uint32_t off = 0; off < n; off += e->pass_max) {
    const uint32_t m = std::min<uint32_t>(e->pass_max, n - off);
    if (int rc = enqueue_chunk(e, rq + (size_t)off * e->msg_size, rp + (size_t)off * e->msg_size, m, &seq, rq_pinned, rp_pinned)) return rc;
  }
  *ticket = seq;
  return 0;
}

int dint_wait(dint_engine_t *e, dint_ticket ticket) {
  if (!e) return fail(DINT_EINVAL, "null engine");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->device));
  if (ticket == 0) return 0;  // nothing was ever submitted
  return wait_seq(e, ticket);
}

int dint_submit(dint_engine_t *e, const void *reqs, uint32_t n, void *replies) {
  dint_ticket t = 0;
  if (int rc = dint_submit_async(e, reqs, n, replies, &t)) return rc;
  return n ? dint_wait(e, t) : 0;
}

int dint_alloc_pinned(size_t bytes, void **out) {
  if (!out) return fail(DINT_EINVAL, "null argument");
  if (hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return fail(DINT_ENOMEM, "hipHostMalloc(%zu)", bytes);
  return 0;
}
void dint_free_pinned(void *p) {
  if (p) hipHostFree(p);
}

// ---- multi-GPU routing ---------------------------------------------------------------------------------------
namespace {
// validate one batch of a routing call, make sure the engine's routing scratch exists, order the stream, fill the job
int route_job(const dint_route_item &it, bool pack, uint64_t cnt_stride, hipStream_t &st, void *stream, dint_route_job *job) {
  dint_engine *e = it.engine;
  if (!e) return fail(DINT_EINVAL, "null engine");
  if (pack && (!it.d_slots || !it.d_cnt || (it.n && (!it.d_reqs || !it.d_slot)))) return fail(DINT_EINVAL, "null argument");
  if (!pack && it.n && (!it.d_slots || !it.d_slot || !it.d_reqs || !it.d_replies)) return fail(DINT_EINVAL, "null argument");
  if (e->cfg.workload == DINT_WL_LOG) return fail(DINT_ESTATE, "workload is not sharded by key");
  if (it.n > DINT_ROUTE_MAXN) return fail(DINT_EINVAL, "at most %u requests per routed batch", DINT_ROUTE_MAXN);
  if (e->shard.count > DINT_ROUTE_MAXW) return fail(DINT_EINVAL, "at most %u shards can be routed to", DINT_ROUTE_MAXW);
  if (it.seg_cap == 0 || (uint64_t)it.seg_cap * e->shard.count > 0xFFFFFFF0ull) return fail(DINT_EINVAL, "bad seg_cap");
  HIP_TRY(hipSetDevice(e->device));
  if (!st) st = stream ? (hipStream_t)stream : e->stream;
  if (pack) {
    if (!e->route.blk) {
      if (int rc = dev_alloc((void **)&e->route.blk, (size_t)2 * DINT_ROUTE_BLK_WORDS * 4)) return rc;
      e->route.blk_next = e->route.blk + DINT_ROUTE_BLK_WORDS;
      HIP_TRY(hipDeviceSynchronize());  // the zero-fill ran on the null stream, which a caller's non-blocking stream does not wait for
    }
    if (int rc = order_route_stream(e, st)) return rc;  // the routing scratch is per engine, and only the routing kernels use it
  }
  job->workload = e->cfg.workload;
  job->msg = e->msg_size;
  job->slots = e->slots_mod;
  job->kv = &e->kv;
  job->shard = e->shard;
  job->d_req = it.d_reqs;
  job->d_rep = it.d_replies;
  job->n = it.n;
  job->d_n = it.d_n;
  job->cap = it.seg_cap;
  job->d_send = it.d_slots;
  job->d_cnt = it.d_cnt;
  job->cnt_stride = cnt_stride;
  job->d_slot = it.d_slot;
  job->rs = e->route;
  job->stats = e->scratch.stats;
  return 0;
}
// every engine of a routing call, each once, locked in address order (two calls that share engines cannot deadlock)
int lock_engines(const dint_route_item *items, uint32_t n_items, std::vector<std::unique_lock<std::mutex>> &locks) {
  std::vector<dint_engine *> es;
  for (uint32_t k = 0; k < n_items; k++) {
    if (!items[k].engine) return fail(DINT_EINVAL, "null engine");
    if (items[k].engine->device != items[0].engine->device) return fail(DINT_EINVAL, "the batches of one call share a device");
    es.push_back(items[k].engine);
  }
  std::sort(es.begin(), es.end());
  es.erase(std::unique(es.begin(), es.end()), es.end());
  for (dint_engine *e : es) locks.emplace_back(e->mu);
  return 0;
}
}  // namespace

int dint_route_pack_multi(const dint_route_item *items, uint32_t n_items, uint64_t seg_stride, uint64_t cnt_stride,
                          void *stream) {
  if (!items || n_items == 0 || n_items > DINT_ROUTE_MAXS) return fail(DINT_EINVAL, "1 .. %u batches per call", DINT_ROUTE_MAXS);
  dint_route_job jobs[DINT_ROUTE_MAXS];
  hipStream_t st = nullptr;
  std::vector<std::unique_lock<std::mutex>> locks;
  if (int rc = lock_engines(items, n_items, locks)) return rc;  // held across the launch: two threads packing with
  if (locks.size() != n_items) return fail(DINT_EINVAL, "an engine routes one batch per call (its routing scratch is one batch's)");
  for (uint32_t k = 0; k < n_items; k++)                        // one engine launch in the order order_route_stream recorded
    if (int rc = route_job(items[k], true, cnt_stride, st, stream, &jobs[k])) return rc;
  dint_launch_route_pack(jobs, n_items, seg_stride, st);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    // some of the per-format launches may be queued already: their tickets and tile words would be left dirty in a
    // copy the engines still point at.  Drain the stream and hand every engine two clean copies again.
    hipStreamSynchronize(st);
    for (uint32_t k = 0; k < n_items; k++) {
      dint_engine *e = items[k].engine;
      hipMemset(std::min(e->route.blk, e->route.blk_next), 0, (size_t)2 * DINT_ROUTE_BLK_WORDS * 4);
      mark_route_stream(e, st);
    }
    hipDeviceSynchronize();
    return fail(DINT_EHIP, "kernel launch: %s", hipGetErrorString(err));
  }
  for (uint32_t k = 0; k < n_items; k++) {
    dint_engine *e = items[k].engine;
    std::swap(e->route.blk, e->route.blk_next);  // the launch left the other copy of the scratch zeroed for the next call
    if (int rc = mark_route_stream(e, st)) return rc;
  }
  return 0;
}

int dint_route_unpack_multi(const dint_route_item *items, uint32_t n_items, uint64_t seg_stride, void *stream) {
  if (!items || n_items == 0 || n_items > DINT_ROUTE_MAXS) return fail(DINT_EINVAL, "1 .. %u batches per call", DINT_ROUTE_MAXS);
  dint_route_job jobs[DINT_ROUTE_MAXS];
  hipStream_t st = nullptr;
  std::vector<std::unique_lock<std::mutex>> locks;
  if (int rc = lock_engines(items, n_items, locks)) return rc;
  for (uint32_t k = 0; k < n_items; k++)
    if (int rc = route_job(items[k], false, 0, st, stream, &jobs[k])) return rc;
  dint_launch_route_unpack(jobs, n_items, seg_stride, st);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(DINT_EHIP, "kernel launch: %s", hipGetErrorString(err));
  return 0;
}

int dint_route_pack(dint_engine_t *e, const void *d_reqs, uint32_t n, void *d_send, uint32_t seg_cap,
                    uint64_t seg_stride, void *d_cnt, uint64_t cnt_stride, uint32_t *d_slot, void *stream) {
  dint_route_item it = {e, d_reqs, n, seg_cap, d_send, d_cnt, d_slot, nullptr, nullptr};
  return dint_route_pack_multi(&it, 1, seg_stride, cnt_stride, stream);
}

int dint_route_unpack(dint_engine_t *e, const void *d_back, uint32_t seg_cap, uint64_t seg_stride,
                      const uint32_t *d_slot, const void *d_reqs, uint32_t n, void *d_replies, void *stream) {
  dint_route_item it = {e, d_reqs, n, seg_cap, const_cast<void *>(d_back), nullptr, const_cast<uint32_t *>(d_slot), d_replies, nullptr};
  return dint_route_unpack_multi(&it, 1, seg_stride, stream);
}

void *dint_engine_stream(dint_engine_t *e) { return e ? (void *)e->stream : nullptr; }
uint32_t dint_max_pass(dint_engine_t *e) { return e ? e->pass_max : 0; }

int dint_stream_wait(dint_engine_t *e, void *other_stream) {
  if (!e) return fail(DINT_EINVAL, "null engine");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->device));
  // one event per engine and direction: a wait captures the state the event had when the wait was enqueued, so
  // recording it again for the next call does not disturb waits that are still pending
  if (!e->ev_wait) HIP_TRY(hipEventCreateWithFlags(&e->ev_wait, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(e->ev_wait, (hipStream_t)other_stream));
  HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_wait, 0));
  return 0;
}

int dint_stream_signal(dint_engine_t *e, void *other_stream) {
  if (!e) return fail(DINT_EINVAL, "null engine");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->device));
  if (!e->ev_signal) HIP_TRY(hipEventCreateWithFlags(&e->ev_signal, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(e->ev_signal, e->stream));
  HIP_TRY(hipStreamWaitEvent((hipStream_t)other_stream, e->ev_signal, 0));
  return 0;
}

int dint_sync(dint_engine_t *e) {
  if (!e) return fail(DINT_EINVAL, "null engine");
  hipStream_t s0, s1, s2;
  HIP_TRY(hipSetDevice(e->device));
  {
    std::lock_guard<std::mutex> lk(e->mu);  // the copy streams are created lazily by the first host submission
    s0 = e->stream; s1 = e->s_h2d; s2 = e->s_d2h;
    // kv engines: the overflow-pool counter travels behind the work on the engine's stream, into the word next to the host path's
    if (e->kv.n_tables)
      HIP_TRY(hipMemcpyAsync(e->h_pool + 1, &e->scratch.stats->pool_exhausted, sizeof(unsigned long long), hipMemcpyDeviceToHost, s0));
  }
  HIP_TRY(hipStreamSynchronize(s0));
  if (s1 && s1 != s0) HIP_TRY(hipStreamSynchronize(s1));
  if (s2 && s2 != s0) HIP_TRY(hipStreamSynchronize(s2));
  // replies of pageable callers that still sit in a slot's page-locked buffer reach the caller's memory here as well (ADVICE r05:
  // a dint_submit_async + dint_sync caller never calls dint_wait)
  std::lock_guard<std::mutex> lk(e->mu);
  for (auto &sl : e->slot)
    if (sl.deliver_to) {
      HIP_TRY(hipEventSynchronize(sl.done));
      slot_deliver(sl);
    }
  // INSERTs of device submissions (dint_submit_device: no dint_wait ever sees them) that found the pool full are reported here,
  // once, as dint_wait reports the host path's (pool_seen and h_pool are compared and updated under e->mu, taken above, as there)
  if (e->kv.n_tables && e->h_pool[1] > e->pool_seen) {
    const unsigned long long lost = e->h_pool[1] - e->pool_seen;
    e->pool_seen = e->h_pool[1];
    if (*e->h_pool < e->h_pool[1]) *e->h_pool = e->h_pool[1];
    return fail(DINT_ENOMEM, "%llu INSERTs found the overflow-entry pool full (dint_config.pool_entries); "
                             "they were answered with a reject code and stored nothing", lost);
  }
  return 0;
}

int64_t dint_read_locks(dint_engine_t *e, uint32_t table, uint32_t *a, uint32_t *b, uint64_t cap) {
  if (!e) return fail(DINT_EINVAL, "null engine");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  if (e->cfg.workload == DINT_WL_FASST || e->cfg.workload == DINT_WL_2PL) {
    uint64_t n = std::min<uint64_t>(cap, e->n_local_slots);
    std::vector<uint2> h(n);
    HIP_TRY(hipMemcpy(h.data(), e->d_lock_tbl, n * sizeof(uint2), hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < n; i++) {
      if (a) a[i] = h[i].x;
      if (b) b[i] = h[i].y;
    }
    return (int64_t)e->n_local_slots;
  }
  if (e->cfg.workload == DINT_WL_TATP || e->cfg.workload == DINT_WL_SMALLBANK) {
    int64_t r = dint_kv_read_locks(&e->kv, table, a, b, cap);
    if (r < 0) return fail((int)r, "bad table %u", table);
    return r;
  }
  return fail(DINT_ESTATE, "workload has no lock table");
}

int64_t dint_read_log(dint_engine_t *e, void *records, uint64_t cap) {
  if (!e) return fail(DINT_EINVAL, "null engine");
  if (!e->log.ring) return fail(DINT_ESTATE, "workload has no log");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  uint64_t n = std::min<uint64_t>(cap, e->log.cap);
  if (records && n) HIP_TRY(hipMemcpy(records, e->log.ring, n * 64, hipMemcpyDeviceToHost));
  uint32_t t[2];
  HIP_TRY(hipMemcpy(t, e->log.tail, sizeof t, hipMemcpyDeviceToHost));
  return (int64_t)t[log_cur(e)];
}

int64_t dint_log_drain(dint_engine_t *e, void *records, uint64_t cap, uint64_t *lost) {
  if (!e || (cap && !records)) return fail(DINT_EINVAL, "null argument");
  if (!e->log.ring) return fail(DINT_ESTATE, "workload has no log");
  std::lock_guard<std::mutex> lk(e->mu);
  return log_drain_locked(e, records, cap, lost, false, nullptr);
}

int64_t dint_log_drain_device(dint_engine_t *e, void *d_records, uint64_t cap, uint64_t *lost, void *stream) {
  if (!e || (cap && !d_records)) return fail(DINT_EINVAL, "null argument");
  if (!e->log.ring) return fail(DINT_ESTATE, "workload has no log");
  std::lock_guard<std::mutex> lk(e->mu);
  return log_drain_locked(e, d_records, cap, lost, true, stream ? (hipStream_t)stream : e->stream);
}

// the ring's words and the drain cursor under passes, announcements, cancels and drains, on the host (include/dint_driver.h): the
// log_ring.h functions ahead_cancel, log_drain_locked and the partition stage call
int64_t dint_log_ring_host(uint32_t cap, const uint32_t *ops, uint32_t n_ops, uint64_t *out, uint64_t out_cap) {
  const int64_t w = lg_walk(cap, ops, n_ops, out, out_cap);
  return w < 0 ? fail(DINT_EINVAL, "dint_log_ring_host: a bad op, a sequence no engine allows, or out too small") : w;
}

// one chunk of dint_log_apply_device: m <= e->replay.cap records at d_rec, everything enqueued on st; the acks are counted
// into e->replay.counts.  timed: the stream is drained and the stage times are added to stage_ms[0..2]
int replay_chunk(dint_engine *e, const void *d_rec, uint32_t m, hipStream_t st, bool timed, double *stage_ms) {
  const uint32_t wl = e->cfg.workload;
  const dint_replay_scratch &r = e->replay;
  if (timed) HIP_TRY(hipEventRecord(e->ev_replay[0], st));
  if (wl == DINT_WL_TATP) {
    // (the sort's temporary storage was sized for a full chunk; a shorter last chunk never needs more)
    if (dint_replay_sort_bytes(m, st) > (int64_t)r.sort_tmp_bytes) return fail(DINT_EHIP, "radix sort: temporary storage too small");
    if (!dint_launch_replay_group(d_rec, m, r, st)) return fail(DINT_EHIP, "radix sort failed");
    if (timed) HIP_TRY(hipEventRecord(e->ev_replay[1], st));
    // the READs, answered in place: one segment whose live count is the word k_replay_probe counted in
    const uint32_t seg_cap = std::max(m, 2u);
    if (int rc = run_pass(e, r.probe, seg_cap, r.probe, st, 0, dint_seg_view(1, seg_cap, (uint64_t)seg_cap * e->msg_size, r.probe_n, 0)))
      return rc;
    e->batches--;  // (not the caller's requests)
    e->requests -= seg_cap;
    dint_launch_replay_emit(d_rec, m, r, st);
  } else {
    if (timed) HIP_TRY(hipEventRecord(e->ev_replay[1], st));
    dint_launch_replay_emit_sb(d_rec, m, r, st);
  }
  if (timed) HIP_TRY(hipEventRecord(e->ev_replay[2], st));
  if (int rc = run_pass(e, r.msgs, m, r.msgs, st)) return rc;
  dint_launch_replay_count(wl, m, r, st);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(DINT_EHIP, "kernel launch: %s", hipGetErrorString(err));
  if (timed) {
    HIP_TRY(hipEventRecord(e->ev_replay[3], st));
    HIP_TRY(hipEventSynchronize(e->ev_replay[3]));
    for (int k = 0; k < 3; k++) {
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, e->ev_replay[k], e->ev_replay[k + 1]));
      stage_ms[k] += ms;
    }
  }
  return 0;
}

int dint_log_apply_device(dint_engine_t *e, const void *d_records, uint64_t n, uint32_t chunk, dint_apply_stats *out) {
  if (!e || (n && !d_records)) return fail(DINT_EINVAL, "null argument");
  const uint32_t wl = e->cfg.workload;
  if (wl != DINT_WL_TATP && wl != DINT_WL_SMALLBANK) return fail(DINT_ESTATE, "workload has no table a log replays into");
  if (e->shard.count > 1 && !shard_replica(e)) return fail(DINT_EINVAL, "a sharded engine: the log would have to be routed first");
  std::lock_guard<std::mutex> lk(e->mu);
  if (int rc = ahead_settle(e)) return rc;
  if (e->ahead.valid) return fail(DINT_ESTATE, "a batch announced by dint_submit_device_ahead is pending");
  HIP_TRY(hipSetDevice(e->device));
  if (chunk == 0 || chunk > e->pass_max) chunk = e->pass_max;
  if (out) memset(out, 0, sizeof *out);
  if (n == 0) return 0;
  if (int rc = replay_alloc(e, (uint32_t)std::min<uint64_t>(chunk, n))) return rc;
  const dint_replay_scratch &r = e->replay;
  hipStream_t st = e->stream;
  if (int rc = order_stream(e, st)) return rc;
  if (shard_replica(e))
    if (int rc = shard_home_check(e, d_records, n, st)) return rc;
  HIP_TRY(hipMemsetAsync(r.counts, 0, 4 * sizeof(unsigned long long), st));
  const bool timed = e->timer.on && out;  // stage times: the stream is drained chunk by chunk (a diagnostic)
  if (timed)
    for (hipEvent_t &ev : e->ev_replay)
      if (!ev) HIP_TRY(hipEventCreate(&ev));
  double stage_ms[3] = {0, 0, 0};
  uint64_t chunks = 0;
  const uint8_t *rec = (const uint8_t *)d_records;
  for (uint64_t off = 0; off < n; off += chunk, chunks++) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - off);
    if (int rc = replay_chunk(e, rec + off * 64, m, st, timed, stage_ms)) return rc;
  }
  if (!out) return 0;
  HIP_TRY(hipStreamSynchronize(st));
  unsigned long long c[3];
  HIP_TRY(hipMemcpy(c, r.counts, sizeof c, hipMemcpyDeviceToHost));
  out->commits = c[0]; out->inserts = c[1]; out->deletes = c[2];
  out->applied = c[0] + c[1] + c[2];
  out->chunks = chunks;
  for (int k = 0; k < 3; k++) out->reserved[k] = (uint64_t)(stage_ms[k] * 1e6);
  return 0;
}

int dint_log_apply_folded_device(dint_engine_t *e, const void *d_records, uint64_t n, uint32_t chunk, uint32_t flags,
                                 dint_fold_stats *out) {
  if (!e || (n && !d_records)) return fail(DINT_EINVAL, "null argument");
  if (flags & ~DINT_FOLD_DRY_RUN) return fail(DINT_EINVAL, "unknown flags %#x", flags);
  if ((uintptr_t)d_records & 15) return fail(DINT_EINVAL, "records: 16-byte aligned");
  const uint32_t wl = e->cfg.workload;
  if (wl != DINT_WL_TATP && wl != DINT_WL_SMALLBANK) return fail(DINT_ESTATE, "workload has no table a log replays into");
  if (e->shard.count > 1 && !shard_replica(e)) return fail(DINT_EINVAL, "a sharded engine: the log would have to be routed first");
  std::lock_guard<std::mutex> lk(e->mu);
  if (int rc = ahead_settle(e)) return rc;
  if (e->ahead.valid) return fail(DINT_ESTATE, "a batch announced by dint_submit_device_ahead is pending");
  HIP_TRY(hipSetDevice(e->device));
  if (chunk == 0 || chunk > e->pass_max) chunk = e->pass_max;
  if (out) memset(out, 0, sizeof *out);
  if (n == 0) return 0;
  const bool dry = (flags & DINT_FOLD_DRY_RUN) != 0;
  const uint32_t cap = (uint32_t)std::min<uint64_t>(chunk, n);
  if (int rc = fold_alloc(e, cap)) return rc;
  if (!dry) {
    if (int rc = replay_alloc(e, cap)) return rc;  // (the deferred records of a chunk: never more than the chunk)
    if (int rc = state_alloc(e, false)) return rc;
  }
  const dint_fold_scratch &f = e->fold;
  hipStream_t st = e->stream;
  if (int rc = order_stream(e, st)) return rc;
  if (shard_replica(e))
    if (int rc = shard_home_check(e, d_records, n, st)) return rc;
  HIP_TRY(hipMemsetAsync(f.counts, 0, DINT_FOLD_COUNTS * sizeof(unsigned long long), st));
  if (!dry) HIP_TRY(hipMemsetAsync(e->replay.counts, 0, 4 * sizeof(unsigned long long), st));
  const bool timed = e->timer.on && out;
  if (timed)
    for (hipEvent_t &ev : e->ev_fold)
      if (!ev) HIP_TRY(hipEventCreate(&ev));
  double ms4[4] = {0, 0, 0, 0};
  uint64_t chunks = 0;
  const uint8_t *rec = (const uint8_t *)d_records;
  for (uint64_t off = 0; off < n; off += chunk, chunks++) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - off);
    const void *d_rec = rec + off * 64;
    if (timed) HIP_TRY(hipEventRecord(e->ev_fold[0], st));
    if (!dint_launch_fold(d_rec, m, wl, e->kv.d_dev, f, st, timed ? e->ev_fold[1] : nullptr)) return fail(DINT_EHIP, "log fold: a sort or scan failed");
    if (int rc = state_launched()) return rc;
    uint32_t w[4];  // {deferred records, repair records, rows}
    HIP_TRY(hipMemcpyAsync(w, f.words, sizeof w, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // the chunk's one wait for its counts
    if (w[0] > m || w[1] > m) return fail(DINT_EHIP, "log fold: counts beyond the chunk");
    if (timed) HIP_TRY(hipEventRecord(e->ev_fold[2], st));
    if (!dry && w[1]) {
      e->blank = false, e->fresh = 0;
      // The fold wrote these records in ascending (table, bucket) order and names no table the workload has not, so the order
      // check cannot fail; its flag is collected with the repair's counts and read once, at the end of the call.
      dint_launch_state_repair_check(e->kv, f.repair, w[1], e->state, st);
      dint_launch_fold_rotate(e->kv.d_dev, st);
      // (the pend set: as dint_state_repair chooses it)
      dint_launch_state_repair(e->kv, f.repair, w[1], (uint32_t)(e->scratch.kvs.pass_no & 1), e->scratch.stats, e->state, st);
      dint_launch_fold_harvest(e->state.words + 8, f, st);
      if (int rc = state_launched()) return rc;
    }
    if (timed) HIP_TRY(hipEventRecord(e->ev_fold[3], st));
    if (!dry && w[0])
      if (int rc = replay_chunk(e, f.def_rec, w[0], st, false, nullptr)) return rc;
    if (timed) {
      HIP_TRY(hipEventRecord(e->ev_fold[4], st));
      HIP_TRY(hipEventSynchronize(e->ev_fold[4]));
      for (int k = 0; k < 4; k++) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, e->ev_fold[k], e->ev_fold[k + 1]));
        ms4[k] += ms;
      }
    }
  }
  HIP_TRY(hipStreamSynchronize(st));
  unsigned long long c[DINT_FOLD_COUNTS], a[3] = {0, 0, 0};
  HIP_TRY(hipMemcpy(c, f.counts, sizeof c, hipMemcpyDeviceToHost));
  if (!dry) HIP_TRY(hipMemcpy(a, e->replay.counts, sizeof a, hipMemcpyDeviceToHost));
  if (out) {
    // folded records: what they would have been; deferred ones: what the replica acked (a dry run: what they would be)
    out->commits = c[0] + (dry ? c[3] : a[0]); out->inserts = c[1] + (dry ? c[4] : a[1]); out->deletes = c[2] + (dry ? c[5] : a[2]);
    out->applied = out->commits + out->inserts + out->deletes;
    out->chunks = chunks;
    out->rows = c[8]; out->deferred_records = c[6]; out->folded_records = n - c[6]; out->deferred_buckets = c[7];
    out->repair_records = c[9];
    out->updated = c[10]; out->inserted = c[11]; out->deleted = c[12]; out->refused = c[13];
    for (int k = 0; k < 4; k++) out->ns[k] = (uint64_t)(ms4[k] * 1e6);
  }
  if (c[14]) return fail(DINT_EHIP, "log fold: repair records out of bucket order (an internal error)");
  if (c[13]) {
    // reported here, as dint_state_repair does: the host path's own check (dint_wait) must not report these inserts a second time
    e->pool_seen += c[13];
    *e->h_pool += c[13];
    if (e->h_pool[1] < e->pool_seen) e->h_pool[1] = e->pool_seen;
    return fail(DINT_ENOMEM, "%llu inserts found the overflow-entry pool full (dint_config.pool_entries); the other records were applied", c[13]);
  }
  return 0;
}

int dint_state_digest(dint_engine_t *e, dint_table_digest *out, uint32_t cap_tables, void *stream) {
  if (!e || !out) return fail(DINT_EINVAL, "null argument");
  if (int rc = state_check(e, true)) return rc;
  if (cap_tables < e->kv.n_tables) return fail(DINT_EINVAL, "%u tables, room for %u", e->kv.n_tables, cap_tables);
  std::lock_guard<std::mutex> lk(e->mu);
  if (int rc = state_quiet(e)) return rc;
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = state_alloc(e, false)) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : e->stream;
  if (int rc = order_stream(e, st)) return rc;
  unsigned long long *d = e->state.words + DINT_STATE_DIGEST_AT;
  dint_launch_state_digest(e->kv, e->state, st);
  if (int rc = state_launched()) return rc;
  if (int rc = mark_stream(e, st)) return rc;
  unsigned long long h[DINT_KV_MAX_TABLES * 4];
  HIP_TRY(hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (uint32_t t = 0; t < e->kv.n_tables; t++) {
    out[t].rows = h[4 * t]; out[t].sum = h[4 * t + 1]; out[t].xr = h[4 * t + 2]; out[t].reserved = 0;
  }
  return (int)e->kv.n_tables;
}

int dint_state_stats(dint_engine_t *e, dint_table_stats *out, uint32_t cap_tables, void *stream) {
  if (!e || !out) return fail(DINT_EINVAL, "null argument");
  if (int rc = state_check(e, true)) return rc;
  if (cap_tables < e->kv.n_tables) return fail(DINT_EINVAL, "%u tables, room for %u", e->kv.n_tables, cap_tables);
  std::lock_guard<std::mutex> lk(e->mu);
  if (int rc = state_quiet(e)) return rc;
  HIP_TRY(hipSetDevice(e->device));
  dint_stats_scratch &s = e->tstats;
  if (!s.part) {
    int rc = dev_alloc((void **)&s.part, (size_t)DINT_KV_MAX_TABLES * DINT_STATE_STATS_GRID * DINT_STATE_STATS_WORDS * sizeof(unsigned long long), false);
    if (!rc) rc = dev_alloc((void **)&s.out, (size_t)DINT_KV_MAX_TABLES * DINT_STATE_STATS_WORDS * sizeof(unsigned long long), false);
    if (rc) {
      hipFree(s.part); hipFree(s.out);
      s = dint_stats_scratch{};
      return rc;
    }
  }
  hipStream_t st = stream ? (hipStream_t)stream : e->stream;
  if (int rc = order_stream(e, st)) return rc;
  dint_launch_state_stats(e->kv, s, st);
  if (int rc = state_launched()) return rc;
  if (int rc = mark_stream(e, st)) return rc;
  static_assert(sizeof(dint_table_stats) == DINT_STATE_STATS_WORDS * sizeof(uint64_t), "a report is a dint_table_stats");
  uint64_t h[DINT_KV_MAX_TABLES][DINT_STATE_STATS_WORDS];
  HIP_TRY(hipMemcpyAsync(h, s.out, sizeof h, hipMemcpyDeviceToHost, st));  // (the one synchronisation of the call)
  HIP_TRY(hipStreamSynchronize(st));
  for (uint32_t t = 0; t < e->kv.n_tables; t++)
    if (st_report_finish(h[t], e->kv.h.tab[t].pool_cap))
      return fail(DINT_ESTATE, "a chain of table %u does not end within %u entries, visits its inline entry twice or leaves the pool: no report", t,
                  KV_MAX_CHAIN);
  memcpy(out, h, (size_t)e->kv.n_tables * sizeof(dint_table_stats));
  return (int)e->kv.n_tables;
}

int64_t dint_state_locks(dint_engine_t *e, void *d_records, uint64_t cap, dint_lock_stats *out, void *stream) {
  if (!e) return fail(DINT_EINVAL, "null engine");
  if (!d_records && cap) return fail(DINT_EINVAL, "no buffer for %llu records", (unsigned long long)cap);
  if ((uintptr_t)d_records & 7) return fail(DINT_EINVAL, "lock records need an 8-byte aligned buffer");
  dint_locks_view v;
  if (int rc = locks_view(e, &v)) return rc;
  std::lock_guard<std::mutex> lk(e->mu);
  if (int rc = state_quiet(e)) return rc;
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = locks_reserve(e, dint_locks_blocks(v))) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : e->stream;
  if (int rc = order_stream(e, st)) return rc;
  dint_launch_locks_list(v, e->tlocks, d_records, cap, st);
  if (int rc = state_launched()) return rc;
  if (int rc = mark_stream(e, st)) return rc;
  unsigned long long h[DINT_LOCKS_WORDS];
  HIP_TRY(hipMemcpyAsync(h, e->tlocks.words, sizeof h, hipMemcpyDeviceToHost, st));  // (the one synchronisation of the call)
  HIP_TRY(hipStreamSynchronize(st));
  dint_lock_stats s;
  memset(&s, 0, sizeof s);
  s.total = h[1];
  for (uint32_t t = 0; t < v.g.n_tables; t++) {
    const unsigned long long *w = h + DINT_LOCKS_SUMS_AT + LK_PART * t;
    s.held[t] = w[LKS_HELD]; s.sum_a += w[LKS_SUM_A]; s.sum_b += w[LKS_SUM_B]; s.no_row += w[LKS_NO_ROW]; s.walk_cut += w[LKS_WALK_CUT];
  }
  if (out) *out = s;
  return (int64_t)(d_records ? std::min<uint64_t>(cap, s.total) : 0);
}

int dint_state_unlock(dint_engine_t *e, const void *d_records, uint64_t n, uint32_t flags, dint_unlock_stats *out, void *stream) {
  if (!e) return fail(DINT_EINVAL, "null engine");
  if (flags & ~(DINT_UNLOCK_ALL | DINT_UNLOCK_DRY_RUN)) return fail(DINT_EINVAL, "unknown flags %#x", flags);
  const bool all = (flags & DINT_UNLOCK_ALL) != 0, dry = (flags & DINT_UNLOCK_DRY_RUN) != 0;
  if (all && (d_records || n)) return fail(DINT_EINVAL, "DINT_UNLOCK_ALL takes no list");
  if (!all && !d_records && n) return fail(DINT_EINVAL, "no list of %llu records", (unsigned long long)n);
  if ((uintptr_t)d_records & 7) return fail(DINT_EINVAL, "lock records need an 8-byte aligned buffer");
  if (n >= LK_MAX_LIST) return fail(DINT_EINVAL, "a list of %llu records: fewer than 2^32 - 16 at a time", (unsigned long long)n);
  dint_locks_view v;
  if (int rc = locks_view(e, &v)) return rc;
  std::lock_guard<std::mutex> lk(e->mu);
  if (int rc = state_quiet(e)) return rc;
  dint_unlock_stats s;
  memset(&s, 0, sizeof s);
  if (!all && n == 0) {
    if (out) *out = s;
    return 0;
  }
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = locks_reserve(e, all ? dint_locks_blocks(v) : dint_locks_list_blocks(n))) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : e->stream;
  if (int rc = order_stream(e, st)) return rc;
  if (all) dint_launch_locks_sweep(v, e->tlocks, dry, st);
  else dint_launch_locks_release(v, e->tlocks, d_records, n, dry, st);
  if (int rc = state_launched()) return rc;
  if (int rc = mark_stream(e, st)) return rc;
  unsigned long long h[DINT_LOCKS_WORDS];
  HIP_TRY(hipMemcpyAsync(h, e->tlocks.words, sizeof h, hipMemcpyDeviceToHost, st));  // (the one synchronisation: verdict and counts)
  HIP_TRY(hipStreamSynchronize(st));
  const unsigned long long *w = h + DINT_LOCKS_SUMS_AT;
  if (all) {
    for (uint32_t t = 0; t < v.g.n_tables; t++, w += LK_PART) {
      s.per_table[t] = w[LKS_HELD]; s.released += w[LKS_HELD]; s.released_a += w[LKS_SUM_A];
      s.released_b += v.g.mode == LK_FASST ? 0 : w[LKS_SUM_B];
    }
  } else {
    if (h[0] != LK_NO_INDEX)
      return fail(DINT_EINVAL, "record %llu: a table or slot the engine has not, a record that holds nothing, or not strictly ascending in (table, "
                               "bucket, q); nothing was released", h[0]);
    for (uint32_t t = 0; t < LK_MAX_TABLES; t++) { s.per_table[t] = w[LKU_TABLE + t]; s.released += w[LKU_TABLE + t]; }
    s.stale = w[LKU_STALE]; s.released_a = w[LKU_REL_A]; s.released_b = w[LKU_REL_B];
  }
  if (out) *out = s;
  return 0;
}

int dint_state_verify(dint_engine_t *e, dint_table_verify *out, uint32_t cap_tables, uint32_t flags, void *stream) {
  if (!e || !out) return fail(DINT_EINVAL, "null argument");
  if (flags & ~DINT_VERIFY_RECLAIM) return fail(DINT_EINVAL, "unknown flags %#x", flags);
  if (int rc = state_check(e, true)) return rc;
  if (cap_tables < e->kv.n_tables) return fail(DINT_EINVAL, "%u tables, room for %u", e->kv.n_tables, cap_tables);
  std::lock_guard<std::mutex> lk(e->mu);
  if (int rc = state_quiet(e)) return rc;
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = dint_verify_alloc(e->kv, e->tverify, flags)) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : e->stream;
  if (int rc = order_stream(e, st)) return rc;
  const bool timed = e->timer.on;  // stage times: a diagnostic, in out[0].reserved[11..13]
  if (timed)
    for (hipEvent_t &ev : e->ev_verify)
      if (!ev) HIP_TRY(hipEventCreate(&ev));
  dint_launch_state_verify(e->kv, e->tverify, flags, st, timed ? e->ev_verify : nullptr);
  if (int rc = state_launched()) return rc;
  if (int rc = mark_stream(e, st)) return rc;
  uint64_t reclaimed = 0;
  const int rc = dint_verify_collect(e->kv, e->tverify, flags, st, out, &reclaimed);  // (the one synchronisation of the call)
  if (reclaimed) e->blank = false, e->fresh = 0;
  if (timed && rc != DINT_EHIP)
    for (int k = 0; k < 3; k++) {
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, e->ev_verify[k], e->ev_verify[k + 1]));
      out[0].reserved[11 + k] = (uint64_t)(ms * 1e6);
    }
  return rc ? rc : (int)e->kv.n_tables;
}

int dint_state_compact(dint_engine_t *e, dint_table_compact *out, uint32_t cap_tables, uint32_t flags, void *stream) {
  if (!e || !out) return fail(DINT_EINVAL, "null argument");
  if (flags & ~DINT_COMPACT_DRY_RUN) return fail(DINT_EINVAL, "unknown flags %#x", flags);
  if (int rc = state_check(e, true)) return rc;
  if (cap_tables < e->kv.n_tables) return fail(DINT_EINVAL, "%u tables, room for %u", e->kv.n_tables, cap_tables);
  std::lock_guard<std::mutex> lk(e->mu);
  if (int rc = state_quiet(e)) return rc;
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = dint_verify_alloc(e->kv, e->tverify, 0)) return rc;
  if (int rc = dint_compact_alloc(e->kv, e->tcompact)) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : e->stream;
  if (int rc = order_stream(e, st)) return rc;
  const bool timed = e->timer.on;  // stage times: a diagnostic, in out[0].reserved[0..3]
  if (timed)
    for (hipEvent_t &ev : e->ev_compact)
      if (!ev) HIP_TRY(hipEventCreate(&ev));
  // (a compaction adds nothing to the tables: a blank engine stays blank, any other stays what it was)
  const int rc = dint_compact_run(e->kv, e->tverify, e->tcompact, flags, st, out, timed ? e->ev_compact : nullptr);
  if (rc == DINT_EHIP) return rc;
  if (int rc2 = mark_stream(e, st)) return rc2;
  if (timed && (rc == 0 || rc == DINT_ESTATE))
    for (int k = 0; k < 4; k++) {
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, e->ev_compact[k], e->ev_compact[k + 1]));
      out[0].reserved[k] = (uint64_t)(ms * 1e6);
    }
  return rc ? rc : (int)e->kv.n_tables;
}

int64_t dint_state_diff(dint_engine_t *a, dint_engine_t *b, void *d_records, uint64_t cap, dint_diff_stats *out, void *stream) {
  if (!a || !b) return fail(DINT_EINVAL, "null engine");
  if (a == b) return fail(DINT_EINVAL, "an engine is not compared with itself");
  if ((cap && !d_records) || ((uintptr_t)d_records & 7)) return fail(DINT_EINVAL, "cap records need an 8-byte aligned buffer");
  if (!a->kv.n_tables || !b->kv.n_tables) return fail(DINT_ESTATE, "workload has no kv table");
  if (a->cfg.workload != b->cfg.workload || a->device != b->device) return fail(DINT_EINVAL, "the engines differ in workload or device");
  for (uint32_t t = 0; t < a->kv.n_tables; t++)
    if (a->kv.hash_size[t] != b->kv.hash_size[t]) return fail(DINT_EINVAL, "the engines differ in n_rows");
  if (int rc = state_check(a, false)) return rc;
  if (int rc = state_check(b, false)) return rc;
  if (a->shard.count != b->shard.count || (a->shard.count > 1 && a->shard.index != b->shard.index))
    return fail(DINT_EINVAL, "the engines differ in shard layout: a shard is compared with the same shard of another set");
  std::unique_lock<std::mutex> l0(*std::min(&a->mu, &b->mu)), l1(*std::max(&a->mu, &b->mu));  // address order
  if (int rc = state_quiet(a)) return rc;
  if (int rc = state_quiet(b)) return rc;
  HIP_TRY(hipSetDevice(a->device));
  if (int rc = state_alloc(a, true)) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : a->stream;
  if (int rc = order_stream(a, st)) return rc;
  if (int rc = order_stream(b, st)) return rc;
  dint_launch_state_diff_count(a->kv, b->kv, a->state, st);
  if (int rc = state_launched()) return rc;
  unsigned long long h[5];
  HIP_TRY(hipMemcpyAsync(h, a->state.words, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (h[4] && d_records && cap) {  // (two engines in sync: one pass over the buckets, nothing to write)
    dint_launch_state_diff_write(a->kv, b->kv, a->state, d_records, cap, st);
    if (int rc = state_launched()) return rc;
  }
  if (int rc = mark_stream(a, st)) return rc;
  if (int rc = mark_stream(b, st)) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  if (out) {
    memset(out, 0, sizeof *out);
    out->total = h[4]; out->only_a = h[0]; out->only_b = h[1]; out->val_differs = h[2]; out->ver_only = h[3];
  }
  return (int64_t)std::min<uint64_t>(h[4], d_records ? cap : 0);
}

// ---- traffic report (k_traffic.hip; traffic_report.h) ---------------------------------------------------------------------------
int dint_traffic_report(dint_engine_t *e, const void *d_reqs, const void *d_replies, uint64_t n, uint32_t top_k, struct dint_traffic_report *out,
                        dint_traffic_key *by_requests, dint_traffic_key *by_rejects, void *stream) {
  if (!e || !out) return fail(DINT_EINVAL, "null argument");
  if (e->cfg.workload == DINT_WL_LOG) return fail(DINT_ESTATE, "a log_server batch has no keys to report");
  if (n > DINT_TRAFFIC_MAX_N) return fail(DINT_EINVAL, "%llu requests: a report takes 2^24 at most", (unsigned long long)n);
  if (top_k > DINT_TRAFFIC_MAX_TOP) return fail(DINT_EINVAL, "top_k %u: %u at most", top_k, DINT_TRAFFIC_MAX_TOP);
  if (top_k && (!by_requests || !by_rejects)) return fail(DINT_EINVAL, "top_k entries need both lists");
  if (n && !d_reqs) return fail(DINT_EINVAL, "n requests need a request array");
  if (n && d_replies == d_reqs) return fail(DINT_EINVAL, "an in-place reply array has lost the requests' types: hand over the pristine requests");
  tr_geom g;
  if (!dint_traffic_geom(e->cfg.workload, e->cfg.n_slots, e->cfg.n_rows, e->cfg.flags, &g)) return fail(DINT_ESTATE, "workload keeps no keys");
  // (tables, pass scratch and an announced batch are not touched: no quiet engine is asked for; the lock orders the call among the
  // engine's other calls on its streams)
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t st = stream ? (hipStream_t)stream : e->stream;
  if (int rc = order_stream(e, st)) return rc;
  dint_traffic_scratch s;  // the call's own temporary memory: allocated by it, freed before it returns -- the engine holds none of it
  const int rc = dint_traffic_run(g, s, d_reqs, d_replies, n, top_k, st, out, by_requests, by_rejects);
  if (rc) (void)hipStreamSynchronize(st);  // (a failed call may have left work queued that reads the scratch)
  dint_traffic_free(s);
  if (int rc2 = mark_stream(e, st)) return rc2;
  return rc;
}

// ---- record routing (k_rroute.hip; state_route.h) -------------------------------------------------------------------------------
int64_t dint_records_route(dint_engine_t *e, uint32_t dst_count, const void *d_records, uint64_t n, void *d_out, uint64_t cap, uint64_t *offsets,
                           void *stream) {
  if (!e || !offsets) return fail(DINT_EINVAL, "null argument");
  if (dst_count == 0 || dst_count > RR_MAX_SHARDS) return fail(DINT_EINVAL, "dst_count %u: 1 .. %u shards", dst_count, RR_MAX_SHARDS);
  if (n && (!d_records || !d_out)) return fail(DINT_EINVAL, "n records need an input and an output buffer");
  if (((uintptr_t)d_records & 15) || ((uintptr_t)d_out & 15)) return fail(DINT_EINVAL, "records and output: 16-byte aligned");
  if (!e->kv.n_tables) return fail(DINT_ESTATE, "workload has no kv table");
  if (n > (1ull << 57)) return fail(DINT_EINVAL, "too many records");
  const uint8_t *src = (const uint8_t *)d_records, *dst = (const uint8_t *)d_out;
  if (n && src < dst + n * 64 && dst < src + n * 64) return fail(DINT_EINVAL, "the input and the output overlap");
  if (rr_tiles(n) * dst_count > RR_MAX_COUNTS) return fail(DINT_EINVAL, "%llu records to %u shards: more (shard, tile) pairs than one scan takes", (unsigned long long)n, dst_count);
  if (cap < n) return fail(DINT_ENOMEM, "%llu records, room for %llu", (unsigned long long)n, (unsigned long long)cap);
  if (n == 0) {
    for (uint32_t h = 0; h <= dst_count; h++) offsets[h] = 0;
    return 0;
  }
  std::lock_guard<std::mutex> lk(e->mu);  // (the scratch is the engine's; its tables are not touched: no quiet engine is asked for)
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = rroute_reserve(e, rr_tiles(n) * dst_count)) return rc;
  rr_geom g;
  g.n_tables = e->kv.n_tables;
  g.n_shards = dst_count;
  for (uint32_t t = 0; t < RR_MAX_TABLES; t++) g.mod[t] = t < e->kv.n_tables ? e->kv.h.mod[t] : dint_make_mod(1);
  hipStream_t st = stream ? (hipStream_t)stream : e->stream;
  if (int rc = order_stream(e, st)) return rc;
  dint_launch_rroute_count(g, d_records, n, e->rroute, st);
  if (int rc = state_launched()) return rc;
  unsigned long long h[DINT_RROUTE_WORDS];
  HIP_TRY(hipMemcpyAsync(h, e->rroute.words, (size_t)(dst_count + 3) * sizeof h[0], hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));  // (the one synchronisation of the call)
  const bool good = h[0] == RR_NO_INDEX && h[2 + dst_count] == n;
  if (good) {
    dint_launch_rroute_write(g, d_records, n, e->rroute, d_out, st);
    if (int rc = state_launched()) return rc;
  }
  if (int rc = mark_stream(e, st)) return rc;
  if (h[0] != RR_NO_INDEX)
    return fail(DINT_EINVAL, "record %llu has no home: its table byte names a table the workload has not; nothing was written", h[0]);
  if (!good) return fail(DINT_EHIP, "record routing: the counts do not add up to the list (an internal error); nothing was written");
  for (uint32_t k = 0; k <= dst_count; k++) offsets[k] = h[2 + k];
  return (int64_t)n;
}

// ---- block sync (k_block.hip; state_block.h) ----------------------------------------------------------------------------------
namespace {
// an upper bound of the buckets n_ids listed blocks hold: tight for a good list (only a table's last block is short)
uint64_t block_lanes_max(const dint_kv &kv, const bk_geom &g, uint32_t n_ids) {
  uint64_t all = 0;
  for (uint32_t t = 0; t < kv.n_tables; t++) all += kv.h.tab[t].n_local;
  return std::max<uint64_t>(1, std::min<uint64_t>(all, (uint64_t)n_ids << g.shift));
}
}  // namespace

int64_t dint_state_block_digest(dint_engine_t *e, uint64_t block_buckets, void *d_out, uint64_t cap_blocks, dint_block_stats *out_stats, void *stream) {
  if (!e) return fail(DINT_EINVAL, "null engine");
  if (int rc = state_check(e, true)) return rc;
  bk_geom g;
  if (!dint_block_geom(e->kv, block_buckets, &g)) return fail(DINT_EINVAL, "block_buckets: a power of two, 64 .. 2^20");
  if ((uintptr_t)d_out & 7) return fail(DINT_EINVAL, "the digests need an 8-byte aligned buffer");
  if (d_out && cap_blocks < bk_blocks(g)) return fail(DINT_EINVAL, "%u blocks, room for %llu", bk_blocks(g), (unsigned long long)cap_blocks);
  std::lock_guard<std::mutex> lk(e->mu);
  if (int rc = state_quiet(e)) return rc;
  dint_block_fill_stats(out_stats, g, bk_blocks(g));
  if (!d_out) return bk_blocks(g);
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = block_reserve(e, g.shift == 6 ? 0 : dint_block_chunks(e->kv), 0, 0, false)) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : e->stream;
  if (int rc = order_stream(e, st)) return rc;
  dint_launch_block_digest(e->kv, g, e->block, d_out, st);
  if (int rc = state_launched()) return rc;
  if (int rc = mark_stream(e, st)) return rc;
  HIP_TRY(hipStreamSynchronize(st));  // (the one synchronisation of the call)
  return bk_blocks(g);
}

int64_t dint_state_block_rows(dint_engine_t *e, uint64_t block_buckets, const void *d_ids, uint32_t n_ids, void *d_records, uint64_t cap,
                              dint_block_stats *out_stats, void *stream) {
  if (!e) return fail(DINT_EINVAL, "null engine");
  if (int rc = state_check(e, true)) return rc;
  bk_geom g;
  if (!dint_block_geom(e->kv, block_buckets, &g)) return fail(DINT_EINVAL, "block_buckets: a power of two, 64 .. 2^20");
  if ((n_ids && !d_ids) || ((uintptr_t)d_ids & 3)) return fail(DINT_EINVAL, "n_ids ids need a 4-byte aligned buffer");
  if ((cap && !d_records) || ((uintptr_t)d_records & 7)) return fail(DINT_EINVAL, "cap records need an 8-byte aligned buffer");
  if (n_ids > bk_blocks(g)) return fail(DINT_EINVAL, "%u ids, %u blocks: %s", n_ids, bk_blocks(g), bk_bad_name(BK_BAD_IDS));
  std::lock_guard<std::mutex> lk(e->mu);
  if (int rc = state_quiet(e)) return rc;
  dint_block_fill_stats(out_stats, g, 0);
  if (n_ids == 0) return 0;
  HIP_TRY(hipSetDevice(e->device));
  const uint64_t lanes = block_lanes_max(e->kv, g, n_ids);
  if (int rc = block_reserve(e, 0, n_ids, lanes, false)) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : e->stream;
  if (int rc = order_stream(e, st)) return rc;
  dint_launch_block_rows_count(e->kv, g, d_ids, n_ids, lanes, e->block, st);
  if (int rc = state_launched()) return rc;
  unsigned long long h[DINT_BLOCK_WORDS];
  HIP_TRY(hipMemcpyAsync(h, e->block.words, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const uint32_t bad = (uint32_t)h[DINT_BLOCK_BAD_AT];
  if (!bad && h[DINT_BLOCK_TOTAL_AT] && d_records && cap) {
    dint_launch_block_rows_write(e->kv, g, d_ids, n_ids, lanes, e->block, d_records, cap, st);
    if (int rc = state_launched()) return rc;
    if (int rc = mark_stream(e, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
  } else if (int rc = mark_stream(e, st)) {
    return rc;
  }
  if (bad) return fail(DINT_EINVAL, "%s; nothing was written", bk_bad_name(bad));
  if (out_stats) out_stats->total = h[DINT_BLOCK_TOTAL_AT];
  return (int64_t)std::min<uint64_t>(h[DINT_BLOCK_TOTAL_AT], d_records ? cap : 0);
}

int64_t dint_state_block_diff(dint_engine_t *e, uint64_t block_buckets, const void *d_ids, uint32_t n_ids, const void *d_rows, uint64_t n_rows,
                              void *d_records, uint64_t cap, dint_diff_stats *out_stats, void *stream) {
  if (!e) return fail(DINT_EINVAL, "null engine");
  if (int rc = state_check(e, true)) return rc;
  bk_geom g;
  if (!dint_block_geom(e->kv, block_buckets, &g)) return fail(DINT_EINVAL, "block_buckets: a power of two, 64 .. 2^20");
  if ((n_ids && !d_ids) || ((uintptr_t)d_ids & 3)) return fail(DINT_EINVAL, "n_ids ids need a 4-byte aligned buffer");
  if ((n_rows && !d_rows) || ((uintptr_t)d_rows & 7) || n_rows > BK_MAX_ROWS) return fail(DINT_EINVAL, "n_rows rows need an 8-byte aligned buffer; fewer than 2^32 - 16");
  if ((cap && !d_records) || ((uintptr_t)d_records & 7)) return fail(DINT_EINVAL, "cap records need an 8-byte aligned buffer");
  if (n_ids > bk_blocks(g)) return fail(DINT_EINVAL, "%u ids, %u blocks: %s", n_ids, bk_blocks(g), bk_bad_name(BK_BAD_IDS));
  if (n_ids == 0 && n_rows) return fail(DINT_EINVAL, "%s; nothing was written", bk_bad_name(BK_BAD_HOME));
  std::lock_guard<std::mutex> lk(e->mu);
  if (int rc = state_quiet(e)) return rc;
  if (out_stats) memset(out_stats, 0, sizeof *out_stats);
  if (n_ids == 0) return 0;
  HIP_TRY(hipSetDevice(e->device));
  const uint64_t lanes = block_lanes_max(e->kv, g, n_ids);
  if (int rc = block_reserve(e, 0, n_ids, lanes, true)) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : e->stream;
  if (int rc = order_stream(e, st)) return rc;
  dint_launch_block_diff_count(e->kv, g, d_ids, n_ids, lanes, d_rows, (uint32_t)n_rows, e->block, st);
  if (int rc = state_launched()) return rc;
  unsigned long long h[DINT_BLOCK_WORDS];
  HIP_TRY(hipMemcpyAsync(h, e->block.words, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const uint32_t bad = (uint32_t)h[DINT_BLOCK_BAD_AT];
  if (!bad && h[DINT_BLOCK_TOTAL_AT] && d_records && cap) {
    dint_launch_block_diff_write(e->kv, g, d_ids, n_ids, lanes, d_rows, (uint32_t)n_rows, e->block, d_records, cap, st);
    if (int rc = state_launched()) return rc;
    if (int rc = mark_stream(e, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
  } else if (int rc = mark_stream(e, st)) {
    return rc;
  }
  if (bad) return fail(DINT_EINVAL, "%s; nothing was written", bk_bad_name(bad));
  if (out_stats) {
    out_stats->total = h[DINT_BLOCK_TOTAL_AT]; out_stats->only_a = h[0]; out_stats->only_b = h[1]; out_stats->val_differs = h[2]; out_stats->ver_only = h[3];
  }
  return (int64_t)std::min<uint64_t>(h[DINT_BLOCK_TOTAL_AT], d_records ? cap : 0);
}

int dint_state_repair(dint_engine_t *e, const void *d_records, uint64_t n, dint_repair_stats *out, void *stream) {
  if (!e || (n && !d_records)) return fail(DINT_EINVAL, "null argument");
  if (((uintptr_t)d_records & 7) || n > 0x7FFFFFFFull * 256ull) return fail(DINT_EINVAL, "records: 8-byte aligned, fewer than 2^39");
  if (int rc = state_check(e, false)) return rc;
  std::lock_guard<std::mutex> lk(e->mu);
  if (int rc = state_quiet(e)) return rc;
  if (out) memset(out, 0, sizeof *out);
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = state_alloc(e, false)) return rc;
  e->blank = false, e->fresh = 0;
  hipStream_t st = stream ? (hipStream_t)stream : e->stream;
  if (int rc = order_stream(e, st)) return rc;
  dint_launch_state_repair_check(e->kv, d_records, n, e->state, st);
  unsigned long long h[5];
  HIP_TRY(hipMemcpyAsync(h, e->state.words + 8, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (h[0]) {
    if (int rc = mark_stream(e, st)) return rc;
    return fail(DINT_EINVAL, "the records are not grouped by bucket (table and bucket ascending, as dint_state_diff writes them), or name "
                             "a table the workload has not; nothing was applied");
  }
  // An emptied overflow entry goes to the pend set the engine's LAST pass pushed to: the pass after next rotates that set
  // (dint_kv_core.h kv_pool_rotate), when this kernel is long over -- never the set the next pass's partition is about to rotate.
  dint_launch_state_repair(e->kv, d_records, n, (uint32_t)(e->scratch.kvs.pass_no & 1), e->scratch.stats, e->state, st);
  if (int rc = state_launched()) return rc;
  if (int rc = mark_stream(e, st)) return rc;
  HIP_TRY(hipMemcpyAsync(h, e->state.words + 8, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (out) {
    out->updated = h[1]; out->inserted = h[2]; out->deleted = h[3]; out->refused = h[4];
    out->applied = h[1] + h[2] + h[3];
  }
  if (h[4]) {
    // reported here: the host path's own check (dint_wait) must not report these inserts a second time
    e->pool_seen += h[4];
    *e->h_pool += h[4];
    if (e->h_pool[1] < e->pool_seen) e->h_pool[1] = e->pool_seen;
    return fail(DINT_ENOMEM, "%llu inserts found the overflow-entry pool full (dint_config.pool_entries); the other records were applied", h[4]);
  }
  return 0;
}

int dint_state_export(dint_engine_t *e, uint32_t dst_index, uint32_t dst_count, void *d_buf, uint64_t cap_bytes, dint_image_stats *out,
                      void *stream) {
  if (!e) return fail(DINT_EINVAL, "null engine");
  if (dst_count == 0) dst_count = 1;
  if (dst_index >= dst_count || dst_count > 255) return fail(DINT_EINVAL, "destination shard %u of %u", dst_index, dst_count);
  if ((uintptr_t)d_buf & 15) return fail(DINT_EINVAL, "an image needs a 16-byte aligned buffer");
  si_header h;
  memset(&h, 0, sizeof h);
  if (!dint_image_shape(e->cfg.workload, &h.n_tables, &h.stride, &h.val_size)) return fail(DINT_ESTATE, "workload has no table");
  const bool lock = !e->kv.n_tables;
  std::lock_guard<std::mutex> lk(e->mu);
  if (int rc = state_quiet(e)) return rc;
  HIP_TRY(hipSetDevice(e->device));
  h.magic = SI_MAGIC; h.version = SI_VERSION; h.workload = e->cfg.workload; h.flags = image_flags(e);
  h.src_index = e->shard.index; h.src_count = e->shard.count; h.dst_index = dst_index; h.dst_count = dst_count;
  si_sel sel[SI_MAX_TABLES];
  uint64_t n_sel[SI_MAX_TABLES] = {0, 0, 0, 0, 0}, n_inl = 0;
  for (uint32_t t = 0; t < h.n_tables; t++) {
    h.table[t].global_size = lock ? e->n_slots : e->kv.hash_size[t];
    sel[t] = si_select(h.table[t].global_size, e->shard.index, e->shard.count, dst_index, dst_count);
    h.table[t].n_buckets = n_sel[t] = sel[t].n;
    n_inl += sel[t].n;
  }
  if (int rc = image_alloc(e, dint_image_blocks(n_sel, h.n_tables), 0, 0)) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : e->stream;
  if (int rc = order_stream(e, st)) return rc;
  const bool write = d_buf && cap_bytes;
  unsigned long long w[DINT_IMAGE_WORDS];
  if (lock) {
    // (one pass: the size does not depend on the table's contents)
    h.table[0].offset = SI_HEADER_BYTES;
    h.bytes = SI_HEADER_BYTES + si_table_bytes(n_sel[0], 0, h.stride, true);
    if (write && cap_bytes < h.bytes) {
      if (out) { memset(out, 0, sizeof *out); out->bytes = h.bytes; out->buckets = n_sel[0]; }
      if (int rc = mark_stream(e, st)) return rc;
      return fail(DINT_ENOMEM, "the image has %llu bytes, the buffer %llu", (unsigned long long)h.bytes, (unsigned long long)cap_bytes);
    }
    dint_launch_image_lock_out(e->d_lock_tbl, sel[0], write ? (uint8_t *)d_buf + SI_HEADER_BYTES : nullptr, e->image, st);
  } else {
    dint_launch_image_count(e->kv, sel, e->image, st);
  }
  if (int rc = state_launched()) return rc;
  HIP_TRY(hipMemcpyAsync(w, e->image.words, sizeof w, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (lock) {
    h.table[0].rows = w[1];
  } else {
    if ((uint32_t)w[DINT_IMAGE_BAD_AT]) {
      if (int rc = mark_stream(e, st)) return rc;
      return fail(DINT_ESTATE, "a chain of the source does not end within %u entries, has more than %u overflow entries or leaves the pool: not exported",
                  KV_MAX_CHAIN, SI_MAX_RUN);
    }
    uint64_t at = SI_HEADER_BYTES;
    for (uint32_t t = 0; t < h.n_tables; t++) {
      h.table[t].n_overflow = w[2 * t]; h.table[t].rows = w[2 * t + 1]; h.table[t].offset = at;
      at += si_table_bytes(n_sel[t], h.table[t].n_overflow, h.stride, false);
    }
    h.bytes = at;
  }
  if (out) {
    memset(out, 0, sizeof *out);
    out->bytes = h.bytes;
    for (uint32_t t = 0; t < h.n_tables; t++) {
      out->buckets += h.table[t].n_buckets; out->overflow_entries += h.table[t].n_overflow; out->rows += h.table[t].rows;
    }
  }
  if (write && !lock && cap_bytes < h.bytes) {
    if (int rc = mark_stream(e, st)) return rc;
    return fail(DINT_ENOMEM, "the image has %llu bytes, the buffer %llu", (unsigned long long)h.bytes, (unsigned long long)cap_bytes);
  }
  if (write) {
    if (!lock) {
      uint64_t n_ovf = 0;
      for (uint32_t t = 0; t < h.n_tables; t++) n_ovf += h.table[t].n_overflow;
      if (int rc = image_alloc(e, 0, n_inl, n_ovf)) return rc;
      dint_launch_image_write(e->kv, sel, h, e->image, (uint8_t *)d_buf, st);
      if (int rc = state_launched()) return rc;
    }
    memcpy(e->h_pinned, &h, sizeof h);  // (the page-locked buffer of dint_load_rows: no host submission is in flight under the lock)
    HIP_TRY(hipMemcpyAsync(d_buf, e->h_pinned, sizeof h, hipMemcpyHostToDevice, st));
  }
  if (int rc = mark_stream(e, st)) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

int dint_state_import(dint_engine_t *e, const void *d_buf, uint64_t bytes, dint_image_stats *out, void *stream) {
  if (!e || !d_buf) return fail(DINT_EINVAL, "null argument");
  if ((uintptr_t)d_buf & 15) return fail(DINT_EINVAL, "an image needs a 16-byte aligned buffer");
  uint32_t n_tables = 0, stride = 0, val_size = 0;
  if (!dint_image_shape(e->cfg.workload, &n_tables, &stride, &val_size)) return fail(DINT_ESTATE, "workload has no table");
  const bool lock = !e->kv.n_tables;
  std::lock_guard<std::mutex> lk(e->mu);
  if (int rc = state_quiet(e)) return rc;
  if (!e->blank) return fail(DINT_ESTATE, "the destination is not blank: dint_reset it first (since creation or reset it has taken requests, rows, a log, a repair or a restore)");
  if (bytes < SI_HEADER_BYTES) return fail(DINT_EINVAL, "image refused: shorter than its header");
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t st = stream ? (hipStream_t)stream : e->stream;
  if (int rc = order_stream(e, st)) return rc;
  si_header h;
  HIP_TRY(hipMemcpyAsync(e->h_pinned, d_buf, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  memcpy(&h, e->h_pinned, sizeof h);
  // from here on the sizes come from this copy of the header, never from the image again
  if (h.magic != SI_MAGIC || h.version != SI_VERSION) return fail(DINT_EINVAL, "image refused: not a state image of this version");
  if (h.workload != e->cfg.workload || h.n_tables != n_tables || h.stride != stride || h.val_size != val_size || h.flags != image_flags(e))
    return fail(DINT_EINVAL, "image refused: workload %u, flags %u; the engine has workload %u, flags %u", h.workload, h.flags, e->cfg.workload,
                image_flags(e));
  if (uint32_t bad = si_header_check(h, bytes, lock)) return fail(DINT_EINVAL, "image refused: %s", si_bad_name(bad));
  if (h.dst_index != e->shard.index || h.dst_count != e->shard.count)
    return fail(DINT_EINVAL, "image refused: addressed to shard %u of %u, this is %u of %u", h.dst_index, h.dst_count, e->shard.index, e->shard.count);
  uint64_t n_b[SI_MAX_TABLES] = {0, 0, 0, 0, 0};
  for (uint32_t t = 0; t < n_tables; t++) {
    const uint64_t global = lock ? e->n_slots : e->kv.hash_size[t], n_local = lock ? e->n_local_slots : e->kv.h.tab[t].n_local;
    if (h.table[t].global_size != global)
      return fail(DINT_EINVAL, "image refused: table %u has %llu global buckets, the engine's %llu", t, (unsigned long long)h.table[t].global_size,
                  (unsigned long long)global);
    if (h.table[t].n_buckets > n_local) return fail(DINT_EINVAL, "image refused: %s", si_bad_name(SI_BAD_SIZE));
    n_b[t] = h.table[t].n_buckets;
  }
  for (const auto &p : e->pieces) {
    if (p.first == h.src_index && p.second == h.src_count) return fail(DINT_ESTATE, "piece (%u of %u) was imported already", h.src_index, h.src_count);
    if (p.second != h.src_count) return fail(DINT_ESTATE, "the destination holds pieces of a source of %u shards, this one is of %u", p.second, h.src_count);
  }
  uint32_t base[SI_MAX_TABLES] = {0, 0, 0, 0, 0};
  for (uint32_t t = 0; t < n_tables && !lock; t++) {
    HIP_TRY(hipMemcpy(&base[t], e->kv.h.tab[t].pool_top, sizeof(uint32_t), hipMemcpyDeviceToHost));
    const uint32_t cap = e->kv.h.tab[t].pool_cap;
    if (base[t] > cap) base[t] = cap;
    if (h.table[t].n_overflow > cap - base[t])
      return fail(DINT_ENOMEM, "table %u: the image has %llu overflow entries, the pool %u free (dint_config.pool_entries)", t,
                  (unsigned long long)h.table[t].n_overflow, cap - base[t]);
  }
  if (int rc = image_alloc(e, dint_image_blocks(n_b, n_tables), 0, 0)) return rc;
  dint_launch_image_check(h, (const uint8_t *)d_buf, lock, e->image, st);
  if (int rc = state_launched()) return rc;
  unsigned long long w[DINT_IMAGE_WORDS];
  HIP_TRY(hipMemcpyAsync(w, e->image.words, sizeof w, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if ((uint32_t)w[DINT_IMAGE_BAD_AT]) {
    if (int rc = mark_stream(e, st)) return rc;
    return fail(DINT_EINVAL, "image refused: %s; no table was touched", si_bad_name((uint32_t)w[DINT_IMAGE_BAD_AT]));
  }
  if (lock) dint_launch_image_lock_in(e->d_lock_tbl, e->n_local_slots, h, (const uint8_t *)d_buf, st);
  else dint_launch_image_import(e->kv, h, (const uint8_t *)d_buf, base, st);
  if (int rc = state_launched()) return rc;
  if (int rc = mark_stream(e, st)) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  e->pieces.push_back({h.src_index, h.src_count});
  if (out) {
    memset(out, 0, sizeof *out);
    out->bytes = bytes;
    for (uint32_t t = 0; t < n_tables; t++) {
      out->buckets += h.table[t].n_buckets; out->overflow_entries += h.table[t].n_overflow; out->rows += w[2 * t + 1];
    }
  }
  return 0;
}

int dint_state_rehash(dint_engine_t *dst, dint_engine_t *const *srcs, uint32_t n_srcs, uint32_t flags, dint_rehash_stats *out, void *stream) {
  if (out) memset(out, 0, sizeof *out);
  if (!dst || !srcs) return fail(DINT_EINVAL, "null argument");
  if (n_srcs == 0 || n_srcs > SR_MAX_SRCS) return fail(DINT_EINVAL, "%u sources: 1 .. %u", n_srcs, SR_MAX_SRCS);
  if (flags & ~DINT_REHASH_DROP_LOCKS) return fail(DINT_EINVAL, "unknown flags %u", flags);
  std::vector<dint_engine *> all{dst};
  for (uint32_t k = 0; k < n_srcs; k++) {
    dint_engine *s = srcs[k];
    if (!s) return fail(DINT_EINVAL, "null engine");
    if (s == dst) return fail(DINT_EINVAL, "the destination is among the sources");
    if (std::find(all.begin(), all.end(), s) != all.end()) return fail(DINT_EINVAL, "source %u appears twice", k);
    all.push_back(s);
  }
  for (dint_engine *e : all)
    if (e->cfg.workload != dst->cfg.workload || image_flags(e) != image_flags(dst) || e->device != dst->device)
      return fail(DINT_EINVAL, "the engines differ in workload, DINT_FLAG_LOCK_SAME_KEY or device");
  if (!dst->kv.n_tables) return fail(DINT_ESTATE, "workload keeps no keys: nothing to rehash (n_slots cannot be changed this way)");
  std::sort(all.begin(), all.end());  // address order
  std::vector<std::unique_lock<std::mutex>> locks;
  for (dint_engine *e : all) locks.emplace_back(e->mu);
  for (dint_engine *e : all)
    if (int rc = state_quiet(e)) return rc;
  if (!dst->blank || !dst->pieces.empty())
    return fail(DINT_ESTATE, "the destination is not blank: dint_reset it first (since creation or reset it has taken requests, rows, a log, a repair, a restore or an image)");
  HIP_TRY(hipSetDevice(dst->device));
  const uint32_t n_tables = dst->kv.n_tables;
  std::vector<const dint_kv *> kvs(n_srcs);
  for (uint32_t k = 0; k < n_srcs; k++) kvs[k] = &srcs[k]->kv;
  const uint32_t nb = dint_rehash_blocks(kvs.data(), n_srcs);
  if (int rc = rehash_alloc(dst, nb, 0, 0, 0)) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : dst->stream;
  for (dint_engine *e : all)
    if (int rc = order_stream(e, st)) return rc;
  auto done = [&](int rc) {  // every way out after the first enqueue
    for (dint_engine *e : all)
      if (int r = mark_stream(e, st)) return r;
    return rc;
  };
  const bool timed = dst->timer.on && out;
  if (timed)
    for (hipEvent_t &ev : dst->ev_rehash)
      if (!ev) HIP_TRY(hipEventCreate(&ev));
  hipEvent_t *ev = dst->ev_rehash;
  // 1. count
  if (timed) HIP_TRY(hipEventRecord(ev[0], st));
  dint_launch_rehash_count(kvs.data(), n_srcs, dst->rehash, st);
  if (timed) HIP_TRY(hipEventRecord(ev[1], st));
  if (int rc = state_launched()) return done(rc);
  unsigned long long w[DINT_REHASH_WORDS];
  HIP_TRY(hipMemcpyAsync(w, dst->rehash.words, sizeof w, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  uint64_t n_row[DINT_KV_MAX_TABLES] = {0, 0, 0, 0, 0}, n_max = 0, n_all = 0, locks_held = 0;
  for (uint32_t t = 0; t < n_tables; t++) {
    n_row[t] = w[DINT_REHASH_TABLE_WORDS * t];
    locks_held += w[DINT_REHASH_TABLE_WORDS * t + 1];
    n_max = std::max(n_max, n_row[t]);
    n_all += n_row[t];
  }
  if (out) { out->rows_seen = n_all; out->locks_held = locks_held; }
  if ((uint32_t)w[DINT_REHASH_BAD_AT] & 1u)
    return done(fail(DINT_ESTATE, "a chain of a source does not end within %u entries or leaves the pool: nothing was placed", KV_MAX_CHAIN));
  if (locks_held && !(flags & DINT_REHASH_DROP_LOCKS))
    return done(fail(DINT_ESTATE, "the sources hold %llu lock words, which cannot follow their keys to another size: release them, or pass "
                                  "DINT_REHASH_DROP_LOCKS", (unsigned long long)locks_held));
  if (n_max > SR_MAX_ROWS) return done(fail(DINT_EINVAL, "a table of %llu rows: at most %llu", (unsigned long long)n_max, (unsigned long long)SR_MAX_ROWS));
  // 2. keys, sort, plan: table by table; what the build needs is kept for every table
  size_t tmp_bytes = 0;
  for (uint32_t t = 0; t < n_tables; t++) {
    if (!n_row[t]) continue;
    const int64_t b = dint_rehash_tmp_bytes(n_row[t], dst->kv.h.tab[t].n_local, st);
    if (b < 0) return done(fail(DINT_EHIP, "radix sort: temporary storage query failed"));
    tmp_bytes = std::max(tmp_bytes, (size_t)b);
  }
  if (int rc = rehash_alloc(dst, nb, n_max, n_all, tmp_bytes)) return done(rc);
  const dint_rehash_scratch &rs = dst->rehash;
  {
    std::vector<const uint8_t *> ptrs((size_t)DINT_KV_MAX_TABLES * SR_MAX_SRCS, nullptr);
    for (uint32_t t = 0; t < n_tables; t++)
      for (uint32_t k = 0; k < n_srcs; k++) ptrs[(size_t)t * SR_MAX_SRCS + k] = kvs[k]->h.tab[t].entries;
    HIP_TRY(hipMemcpyAsync(rs.src_entries, ptrs.data(), ptrs.size() * sizeof(uint8_t *), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // (a pageable source that goes out of scope)
  }
  uint64_t row_at[DINT_KV_MAX_TABLES] = {0, 0, 0, 0, 0};
  uint32_t blk_at = 0;
  for (uint32_t t = 0; t < n_tables; t++) {
    row_at[t] = t ? row_at[t - 1] + n_row[t - 1] : 0;
    if (n_row[t] && !dint_launch_rehash_plan(t, kvs.data(), n_srcs, blk_at, dst->kv, n_row[t], row_at[t], rs, st, timed ? ev + 4 + 4 * t : nullptr))
      return done(fail(DINT_EHIP, "radix sort or scan failed"));
    for (uint32_t k = 0; k < n_srcs; k++) blk_at += (uint32_t)((kvs[k]->h.tab[t].n_local + 255) / 256);
  }
  if (int rc = state_launched()) return done(rc);
  HIP_TRY(hipMemcpyAsync(w, rs.words, sizeof w, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  uint64_t n_ent[DINT_KV_MAX_TABLES] = {0, 0, 0, 0, 0}, need[DINT_KV_MAX_TABLES] = {0, 0, 0, 0, 0}, placed = 0;
  int short_t = -1;
  for (uint32_t t = 0; t < n_tables; t++) {
    const unsigned long long *wt = w + DINT_REHASH_TABLE_WORDS * t;
    n_ent[t] = wt[2] >> 32; need[t] = wt[2] & 0xFFFFFFFFull;
    placed += wt[3];
    if (out) { out->table[t].rows = wt[3]; out->table[t].overflow_entries = need[t]; out->table[t].longest_chain = wt[4]; }
    if (short_t < 0 && need[t] > dst->kv.h.tab[t].pool_cap) short_t = (int)t;
  }
  if (out) { out->rows_placed = placed; out->rows_foreign = n_all - placed; }
  if ((uint32_t)w[DINT_REHASH_BAD_AT] & 2u)
    return done(fail(DINT_ESTATE, "a bucket of the destination would need more than %u overflow entries: nothing was placed (a larger n_rows)", SI_MAX_RUN));
  if (short_t >= 0)
    return done(fail(DINT_ENOMEM, "table %d needs %llu overflow entries, the destination's pool has %u (dint_config.pool_entries); nothing was placed",
                     short_t, (unsigned long long)need[short_t], dst->kv.h.tab[short_t].pool_cap));
  // 3. build
  if (timed) HIP_TRY(hipEventRecord(ev[2], st));
  for (uint32_t t = 0; t < n_tables; t++)
    dint_launch_rehash_build(t, dst->kv, n_row[t], row_at[t], n_ent[t], (uint32_t)need[t], rs.src_entries + (size_t)t * SR_MAX_SRCS, rs, st);
  if (timed) HIP_TRY(hipEventRecord(ev[3], st));
  dst->blank = false, dst->fresh = 0;
  if (int rc = state_launched()) return done(rc);
  if (int rc = done(0)) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  if (timed) {
    auto ns = [](hipEvent_t a, hipEvent_t b) {
      float ms = 0;
      return hipEventElapsedTime(&ms, a, b) == hipSuccess ? (uint64_t)(ms * 1e6) : 0ull;
    };
    out->stage_ns[0] = ns(ev[0], ev[1]);
    for (uint32_t t = 0; t < n_tables; t++)
      if (n_row[t])
        for (int k = 0; k < 3; k++) out->stage_ns[1 + k] += ns(ev[4 + 4 * t + k], ev[4 + 4 * t + k + 1]);
    out->stage_ns[4] = ns(ev[2], ev[3]);
  }
  return 0;
}

int dint_refuse(uint32_t workload, const void *reqs, uint32_t n, void *replies) {
  if (workload >= DINT_WL_COUNT || (n && (!reqs || !replies))) return fail(DINT_EINVAL, "bad argument");
  const uint32_t msg = kMsgSize[workload];
  const uint8_t *rq = (const uint8_t *)reqs;
  uint8_t *rp = (uint8_t *)replies;
  if (rp != rq) memcpy(rp, rq, (size_t)n * msg);
  for (uint32_t i = 0; i < n; i++) {
    uint8_t *m = rp + (size_t)i * msg;
    switch (workload) {
      case DINT_WL_2PL:  // RETRY, lock_2pl/ebpf/ls_kern.c:59-64
        m[0] = 4;
        break;
      case DINT_WL_STORE:  // kRejectRead / kRejectSet / kRejectInsert, store/ebpf/store_kern.c:57-62
        if (m[0] <= 2) m[0] = (uint8_t)(4 + 2 * m[0] + (m[0] == 2));  // 0 -> 4, 1 -> 6, 2 -> 9
        break;
      case DINT_WL_TATP:  // REJECT_READ / REJECT_LOCK / REJECT_COMMIT, tatp/ebpf/shard_kern.c:173-178,289-293,371-376
        if (m[1] == 0) m[1] = 5;
        else if (m[1] == 1) m[1] = 8;
        else if (m[1] == 12 || m[1] == 13 || m[1] == 18 || m[1] == 19 || m[1] == 22 || m[1] == 23) m[1] = 11;
        break;  // ABORT and the log appends are never refused by the eBPF server either
      case DINT_WL_SMALLBANK:  // RETRY, smallbank/ebpf/shard_kern.c:96-110,603-608
        if (m[1] <= 5 || m[1] == 17) m[1] = 16;
        break;
      default:  // lock_fasst: REJECT_LOCK is the only "not now" a client understands; the log server has none
        if (workload == DINT_WL_FASST && m[0] == 1) m[0] = 6;
        break;
    }
  }
  return 0;
}

int dint_get_stats(dint_engine_t *e, dint_stats *out) {
  if (!e || !out) return fail(DINT_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  dint_dev_stats d;
  HIP_TRY(hipMemcpy(&d, e->scratch.stats, sizeof d, hipMemcpyDeviceToHost));
  memset(out, 0, sizeof *out);
  out->batches = e->batches;
  out->requests = e->requests;
  out->bad_requests = d.bad_requests;
  out->missing_keys = d.missing_keys;
  out->foreign_requests = d.foreign_requests;
  out->pool_exhausted = d.pool_exhausted;
  out->route_overflow = d.route_overflow;
  out->big_bin_requests = d.big_bin_requests;
  out->late_requests = d.late_requests;
  for (int k = 0; k < 3; k++) out->reserved[k] = d.late_items[k];  // (diagnostic: late work items by kind -- sub / solo / pieces)
  return 0;
}

int dint_reset(dint_engine_t *e) {
  if (!e) return fail(DINT_EINVAL, "null engine");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  if (int rc = ahead_cancel(e)) return rc;
  for (auto &r : e->regions) HIP_TRY(hipMemset(r.first, 0, r.second));
  e->blank = true, e->fresh = ~0u;
  e->pieces.clear();
  e->batches = e->requests = 0;
  e->log_drained = e->log_gone = 0;
  e->pool_seen = 0;
  e->h_pool[0] = e->h_pool[1] = 0;
  HIP_TRY(hipDeviceSynchronize());
  return 0;
}

int dint_snapshot(dint_engine_t *e) {
  if (!e) return fail(DINT_EINVAL, "null engine");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  if (int rc = ahead_settle(e)) return rc;
  if (e->ahead.valid) return fail(DINT_ESTATE, "a batch announced by dint_submit_device_ahead is pending (its log records are appended)");
  if (e->kv.n_tables && e->log.tail) {  // both tail words say where the ring stands: whatever the parity of the passes after a restore
    uint32_t t[2];
    HIP_TRY(hipMemcpy(t, e->log.tail, sizeof t, hipMemcpyDeviceToHost));
    t[0] = t[1] = t[log_cur(e)];
    HIP_TRY(hipMemcpy(e->log.tail, t, sizeof t, hipMemcpyHostToDevice));
  }
  if (e->snap.empty()) {
    for (auto &r : e->regions) {
      void *p = nullptr;
      int rc = dev_alloc(&p, r.second, false);
      if (rc) return rc;
      e->snap.push_back(p);
    }
  }
  for (size_t i = 0; i < e->regions.size(); i++)
    HIP_TRY(hipMemcpy(e->snap[i], e->regions[i].first, e->regions[i].second, hipMemcpyDeviceToDevice));
  HIP_TRY(hipDeviceSynchronize());
  e->snap_log_drained = e->log_drained;
  return 0;
}

int dint_restore(dint_engine_t *e) {
  if (!e) return fail(DINT_EINVAL, "null engine");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->snap.empty()) return fail(DINT_ESTATE, "no snapshot taken");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  if (int rc = ahead_cancel(e)) return rc;
  e->blank = false, e->fresh = 0;
  for (size_t i = 0; i < e->regions.size(); i++)
    HIP_TRY(hipMemcpy(e->regions[i].first, e->snap[i], e->regions[i].second, hipMemcpyDeviceToDevice));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(e->h_pool, &e->scratch.stats->pool_exhausted, sizeof(unsigned long long), hipMemcpyDeviceToHost));
  e->pool_seen = e->h_pool[1] = *e->h_pool;
  e->log_gone = 0;
  e->log_drained = e->snap_log_drained;  // the drain cursor belongs to the log's history
  return 0;
}

int dint_load_rows(dint_engine_t *e, uint32_t table, const uint64_t *keys, const uint32_t *vers, const void *vals,
                   uint64_t n) {
  if (!e || (n && (!keys || !vals))) return fail(DINT_EINVAL, "null argument");
  if (!e->kv.n_tables) return fail(DINT_ESTATE, "workload has no kv table");
  if (table >= e->kv.n_tables) return fail(DINT_EINVAL, "bad table %u", table);
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->device));
  return load_rows_locked(e, table, keys, vers, (const uint8_t *)vals, n);
}

int dint_populate(dint_engine_t *e, uint64_t populate_n) {
  if (!e) return fail(DINT_EINVAL, "null engine");
  if (!e->kv.n_tables) return fail(DINT_ESTATE, "workload has no kv table");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->device));
  return dint_pop::generate(e->cfg.workload, populate_n,
                            [e](uint32_t table, const uint64_t *keys, const uint8_t *vals, uint64_t n) {
                              return load_rows_locked(e, table, keys, nullptr, vals, n);
                            });
}

namespace {

uint64_t event_ns(hipEvent_t a, hipEvent_t b) {
  float ms = 0;
  return hipEventElapsedTime(&ms, a, b) == hipSuccess ? (uint64_t)(ms * 1e6) : 0ull;
}

// n rows of device arrays into `table`, under the engine's mutex and behind state_quiet: directly where the table has taken
// nothing, else as load-mode passes formed on the device.  extra_bytes: temporary memory the caller holds (the rows themselves)
int load_device_locked(dint_engine *e, uint32_t table, const uint64_t *d_keys, const uint32_t *d_vers, const void *d_vals, uint64_t n,
                       dint_load_stats *out, hipStream_t st, size_t extra_bytes) {
  const bool direct = (e->fresh >> table & 1u) && e->pieces.empty();
  const kv_tab &tb = e->kv.h.tab[table];
  auto peak = [&]() {
    if (out) out->temp_bytes = std::max<uint64_t>(out->temp_bytes, extra_bytes + load_scratch_bytes(e->load));
  };
  if (out) out->table[table].direct = direct;
  if (!n) return 0;
  if (!direct) {
    if (out) out->direct = 0;
    if (int rc = load_alloc(e, 0, 0)) return rc;
    peak();
    if (int rc = order_stream(e, st)) return rc;
    dint_launch_load_count(e->kv, table, d_keys, n, e->load, st);
    if (int rc = state_launched()) return rc;
    for (uint64_t off = 0; off < n; off += e->pass_max) {
      const uint32_t m = (uint32_t)std::min<uint64_t>(e->pass_max, n - off);
      dint_launch_load_msgs(e->kv, table, d_keys, d_vers, d_vals, off, m, e->slot[0].d_req, st);
      if (int rc = run_pass(e, e->slot[0].d_req, m, e->slot[0].d_req, st, 1)) return rc;
      e->batches--;  // population passes are not request batches
      e->requests -= m;
    }
    unsigned long long foreign = 0;
    HIP_TRY(hipMemcpyAsync(&foreign, e->load.words + DINT_LOAD_FOREIGN_AT, sizeof foreign, hipMemcpyDeviceToHost, st));
    if (int rc = mark_stream(e, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    if (out) {
      out->table[table].rows += n - foreign;
      out->rows_loaded += n - foreign;
      out->foreign_rows += foreign;
    }
    return 0;
  }
  if (tb.n_local >= 0xFFFFFFFFull) return fail(DINT_EINVAL, "table %u has %llu local buckets: the sort keys are 32-bit", table, (unsigned long long)tb.n_local);
  const int64_t tmp = dint_load_tmp_bytes(n, tb.n_local, st);
  if (tmp < 0) return fail(DINT_EHIP, "radix sort: temporary storage query failed");
  if (int rc = load_alloc(e, n, (size_t)tmp)) return rc;
  peak();
  const bool timed = e->timer.on && out;
  if (timed)
    for (hipEvent_t &ev : e->ev_load)
      if (!ev) HIP_TRY(hipEventCreate(&ev));
  hipEvent_t *ev = e->ev_load;
  if (int rc = order_stream(e, st)) return rc;
  auto done = [&](int rc) {  // every way out after the first enqueue
    if (int r = mark_stream(e, st)) return r;
    return rc;
  };
  if (!dint_launch_load_plan(e->kv, table, d_keys, n, e->load, st, timed ? ev : nullptr)) return done(fail(DINT_EHIP, "radix sort or scan failed"));
  if (int rc = state_launched()) return done(rc);
  unsigned long long w[DINT_LOAD_WORDS];
  HIP_TRY(hipMemcpyAsync(w, e->load.words, sizeof w, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const uint64_t n_ent = w[DINT_LOAD_TOTAL_AT] >> 32, need = w[DINT_LOAD_TOTAL_AT] & 0xFFFFFFFFull;
  if (out) {
    out->table[table].overflow_entries = need;
    out->table[table].longest_chain_entries = w[DINT_LOAD_LONGEST_AT];
  }
  if ((uint32_t)w[DINT_LOAD_BAD_AT] & 2u)
    return done(fail(DINT_ESTATE, "a bucket of table %u would need more than %u overflow entries: nothing was written (a larger n_rows)", table, KV_MAX_CHAIN - 1u));
  if (need > tb.pool_cap)
    return done(fail(DINT_ENOMEM, "table %u needs %llu overflow entries, the pool has %u (dint_config.pool_entries); nothing was written", table,
                     (unsigned long long)need, tb.pool_cap));
  dint_launch_load_build(e->kv, table, d_keys, d_vers, d_vals, n, n_ent, (uint32_t)need, e->load, st);
  if (timed) HIP_TRY(hipEventRecord(ev[4], st));
  e->blank = false;
  e->fresh &= ~(1u << table);
  if (int rc = state_launched()) return done(rc);
  if (int rc = done(0)) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  if (out) {
    out->table[table].rows += n - w[DINT_LOAD_FOREIGN_AT];
    out->rows_loaded += n - w[DINT_LOAD_FOREIGN_AT];
    out->foreign_rows += w[DINT_LOAD_FOREIGN_AT];
    if (timed)
      for (int k = 0; k < 4; k++) out->stage_ns[1 + k] += event_ns(ev[k], ev[k + 1]);
  }
  return 0;
}

}  // namespace

int dint_load_rows_device(dint_engine_t *e, uint32_t table, const uint64_t *d_keys, const uint32_t *d_vers, const void *d_vals, uint64_t n,
                          dint_load_stats *out, void *stream) {
  if (out) memset(out, 0, sizeof *out);
  if (!e || (n && (!d_keys || !d_vals))) return fail(DINT_EINVAL, "null argument");
  if (!e->kv.n_tables) return fail(DINT_ESTATE, "workload has no kv table");
  if (table >= e->kv.n_tables) return fail(DINT_EINVAL, "bad table %u", table);
  if (((uintptr_t)d_keys & 7) || ((uintptr_t)d_vers & 3) || ((uintptr_t)d_vals & 7))
    return fail(DINT_EINVAL, "keys and values need 8-byte aligned arrays, versions a 4-byte aligned one");
  if (n > SR_MAX_ROWS) return fail(DINT_EINVAL, "%llu rows: at most %llu a call", (unsigned long long)n, (unsigned long long)SR_MAX_ROWS);
  std::lock_guard<std::mutex> lk(e->mu);
  if (int rc = state_quiet(e)) return rc;
  HIP_TRY(hipSetDevice(e->device));
  if (out) out->direct = 1;
  return load_device_locked(e, table, d_keys, d_vers, d_vals, n, out, stream ? (hipStream_t)stream : e->stream, 0);
}

int dint_populate_device(dint_engine_t *e, uint64_t populate_n, dint_load_stats *out, void *stream) {
  if (out) memset(out, 0, sizeof *out);
  if (!e) return fail(DINT_EINVAL, "null engine");
  if (!e->kv.n_tables) return fail(DINT_ESTATE, "workload has no kv table");
  if (populate_n > SR_MAX_ROWS / 12) return fail(DINT_EINVAL, "%llu subscribers: a table's rows must stay below 2^32 - 16", (unsigned long long)populate_n);
  std::lock_guard<std::mutex> lk(e->mu);
  if (int rc = state_quiet(e)) return rc;
  if (!e->blank || !e->pieces.empty())
    return fail(DINT_ESTATE, "the engine is not blank: dint_reset it first (since creation or reset it has taken requests, rows, a log, a repair, a restore or an image)");
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t st = stream ? (hipStream_t)stream : e->stream;
  const uint32_t wl = e->cfg.workload, vs = e->kv.val_size;
  if (out) out->direct = 1;
  // the tile tables of the two data-dependent tatp groups, walked on another core while the device loads the tables that need none
  struct Prepass { int rc = 0; uint64_t ns = 0; };
  std::future<Prepass> pre;
  if (wl == DINT_WL_TATP)
    pre = std::async(std::launch::async, [populate_n]() {
      Prepass p;
      const auto t0 = std::chrono::steady_clock::now();
      p.rc = dint_load_tiles(SL_G_AI, 0, populate_n, nullptr, nullptr, nullptr);
      if (!p.rc) p.rc = dint_load_tiles(SL_G_SFCF, 0, populate_n, nullptr, nullptr, nullptr);
      p.ns = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
      return p;
    });
  const bool timed = e->timer.on && out;
  if (timed)
    for (hipEvent_t &ev : e->ev_load)
      if (!ev) HIP_TRY(hipEventCreate(&ev));
  int rc = 0;
  for (uint32_t t = 0; t < e->kv.n_tables && !rc; t++) {
    uint32_t which;
    const uint32_t group = sl_group(wl, t, &which);
    uint64_t rows = populate_n * sl_rows_fixed(group);
    std::vector<uint64_t> tile_state, tile_rows;
    if (sl_draws(group) == SL_DRAWS_VAR) {
      if (pre.valid()) {
        const Prepass p = pre.get();
        if (p.rc) { rc = fail(p.rc, "the tile table of the population could not be built"); break; }
        if (out) out->stage_ns[5] = p.ns;
      }
      if ((rc = dint_load_tiles(group, which, populate_n, &tile_state, &tile_rows, &rows))) { rc = fail(rc, "the tile table of the population could not be built"); break; }
    }
    if (!rows) continue;
    uint64_t *d_keys = nullptr, *d_tiles = nullptr;
    void *d_vals = nullptr;
    const size_t tile_bytes = tile_state.size() * 2 * sizeof(uint64_t), row_bytes = (size_t)rows * (8 + vs);
    rc = dev_alloc((void **)&d_keys, (size_t)rows * 8, false);
    if (!rc) rc = dev_alloc(&d_vals, (size_t)rows * vs, false);
    if (!rc && tile_bytes) rc = dev_alloc((void **)&d_tiles, tile_bytes, false);
    if (!rc && tile_bytes) {
      hipError_t he = hipMemcpy(d_tiles, tile_state.data(), tile_bytes / 2, hipMemcpyHostToDevice);
      if (he == hipSuccess) he = hipMemcpy(d_tiles + tile_state.size(), tile_rows.data(), tile_bytes / 2, hipMemcpyHostToDevice);
      if (he != hipSuccess) rc = fail(DINT_EHIP, "hipMemcpy: %s", hipGetErrorString(he));
    }
    if (!rc) rc = order_stream(e, st);
    if (!rc) {
      if (timed) (void)hipEventRecord(e->ev_load[5], st);
      dint_launch_load_gen(group, which, populate_n, d_tiles, d_tiles ? d_tiles + tile_state.size() : nullptr, d_keys, d_vals, rows, vs, st);
      rc = state_launched();
    }
    if (!rc) rc = load_device_locked(e, t, d_keys, nullptr, d_vals, rows, out, st, row_bytes + tile_bytes);
    if (!rc && timed) out->stage_ns[0] += event_ns(e->ev_load[5], e->ev_load[0]);
    (void)hipStreamSynchronize(st);
    hipFree(d_keys); hipFree(d_vals); hipFree(d_tiles);
  }
  if (pre.valid()) pre.wait();
  load_free(e);
  return rc;
}

int64_t dint_hash_size(dint_engine_t *e, uint32_t table) {
  if (!e) return fail(DINT_EINVAL, "null engine");
  if (table >= e->kv.n_tables) return fail(DINT_EINVAL, "bad table %u", table);
  return (int64_t)e->kv.hash_size[table];
}

int64_t dint_dump_rows(dint_engine_t *e, uint32_t table, uint64_t *keys, uint32_t *vers, void *vals, uint64_t cap) {
  if (!e) return fail(DINT_EINVAL, "null engine");
  if (table >= e->kv.n_tables) return fail(DINT_EINVAL, "bad table %u", table);
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  return dint_kv_dump_rows(&e->kv, table, keys, vers, (uint8_t *)vals, cap);
}

int dint_home_shard(dint_engine_t *e, const void *d_reqs, uint32_t n, uint8_t *d_home, void *stream) {
  if (!e || (n && (!d_reqs || !d_home))) return fail(DINT_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t st = stream ? (hipStream_t)stream : e->stream;
  switch (e->cfg.workload) {
    case DINT_WL_FASST:
    case DINT_WL_2PL:
      dint_launch_home_lid(d_reqs, e->msg_size, n, e->slots_mod, e->shard.count, d_home, st);
      break;
    case DINT_WL_STORE:
    case DINT_WL_TATP:
    case DINT_WL_SMALLBANK:
      dint_launch_home_kv(d_reqs, n, e->kv, d_home, st);
      break;
    default:
      return fail(DINT_ESTATE, "workload is not sharded by key");
  }
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(DINT_EHIP, "kernel launch: %s", hipGetErrorString(err));
  return 0;
}

int dint_kv_trace_read(dint_engine_t *e, uint64_t *out, uint64_t cap) {
  if (!e || !out) return fail(DINT_EINVAL, "null argument");
  if (!e->kv.d_trace) return fail(DINT_ESTATE, "tracing is off (set DINT_KV_TRACE=1 before creating the engine)");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  const uint64_t words = std::min<uint64_t>(cap, (uint64_t)DINT_KV_TRACE_WORDS);
  HIP_TRY(hipMemcpy(out, e->kv.d_trace, words * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(e->kv.d_trace, 0, DINT_KV_TRACE_WORDS * 8));  // the next read sees one launch only
  HIP_TRY(hipDeviceSynchronize());  // (a fill on the null stream: the engine's streams do not wait for it)
  return (int)DINT_KV_PMAX;
}

int dint_timing_enable(dint_engine_t *e, int on) {
  if (!e) return fail(DINT_EINVAL, "null engine");
  std::lock_guard<std::mutex> lk(e->mu);
  e->timer.on = on != 0;
  e->timer.passes = 0;
  return 0;
}

int dint_timing_read(dint_engine_t *e, const char **names, double *avg_us, uint64_t *launches, int cap) {
  if (!e) return fail(DINT_EINVAL, "null engine");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  KernelTimer &t = e->timer;
  int nk = std::min(t.n_kernels, cap);
  for (int k = 0; k < nk; k++) {
    double sum = 0;
    for (int p = 0; p < t.passes; p++) {
      float ms = 0;
      hipEvent_t *ev = &t.ev[(size_t)p * (t.n_kernels + 1)];
      if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess) sum += ms;
    }
    names[k] = t.names[k];
    avg_us[k] = t.passes ? sum * 1000.0 / t.passes : 0.0;
    launches[k] = (uint64_t)t.passes;
  }
  t.passes = 0;
  return nk;
}

}  // extern "C"
