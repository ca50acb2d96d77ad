// k_lock_client.hip -- the lock micro-benchmarks' load generators resident on the GPU (include/dint_driver.h
// dint_lock_gclient_*).
//
// The callers of lock_fasst / lock_2pl -- lock_fasst/caladan/client.cc:183-280, lock_2pl/caladan/client.cc:167-240 -- as
// device code: the SAME worker state machines the host clients run (lock_clients.h is compiled for both), one lane per
// worker.  A worker has one request outstanding, so request i of an epoch belongs to worker i: no scan, unlike k_txn_emit.
//
//   k_lock_client : every worker takes the reply to its last request (consume) and/or emits its next request (emit).  When
//                   consume and the next emit are issued on the same stream (the closed loop does) they are ONE launch: the
//                   epoch's batch alternates between two buffers, so a worker reads the reply of epoch k from one while the
//                   request of epoch k + 1 goes into the other.  DINT_LOCK_CLIENT_FUSE=0 keeps a consume kernel of its own.
//
// Worker state lives in HBM as dword COLUMNS (word j of worker i at cols[j * n + i], as k_txn.hip keeps its client
// headers): the header (lock_clients.h LcState, one dword), the RNG (two), the transaction's ten keys and, for lock_fasst,
// the ten versions it read.  Per epoch a lane loads and stores its header and touches the key or version its step needs
// (lock_fasst: the key it sent, to check the reply's lid, and the key it sends next; a version on READ / VALIDATE); the
// RNG and the key set only when a transaction starts.  The messages (9 / 6 bytes, unaligned) pass through LDS, so the
// batch is read and written in whole 16-byte vectors.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "../../include/dint_abi.h"
#include "../../include/dint_driver.h"
#include "lock_clients.h"

#define LCG_TB 256u   // workers per workgroup
#define LCG_RNG 1u    // columns: 0 header, 1-2 RNG (low, high word), 3-12 keys, 13-22 versions (lock_fasst)
#define LCG_KEYS 3u
#define LCG_VERS 13u
#define LCG_NSTAT 4   // committed, rejects, rollbacks, protocol_errors

int dint_lock_client_params(const dint_fasst_client_config *cfg, LcParams *P, ZipfTable *zipf);  // fasst_client.cc

static_assert(sizeof(dint_lock_client_config) == sizeof(dint_fasst_client_config) &&
                  offsetof(dint_lock_client_config, zipf_theta) == offsetof(dint_fasst_client_config, zipf_theta),
              "dint_lock_client_config is dint_fasst_client_config with the workload in reserved0");

struct LcCols {  // lock_clients.h storage: worker i's words in the columns
  uint32_t *c;
  uint32_t n, i;
  __device__ uint32_t &at(uint32_t col) const { return c[(size_t)col * n + i]; }
  __device__ uint64_t rng() const { return at(LCG_RNG) | (uint64_t)at(LCG_RNG + 1) << 32; }
  __device__ void set_rng(uint64_t v) const { at(LCG_RNG) = (uint32_t)v; at(LCG_RNG + 1) = (uint32_t)(v >> 32); }
  __device__ uint32_t key(uint32_t j) const { return at(LCG_KEYS + j); }
  __device__ void set_key(uint32_t j, uint32_t v) const { at(LCG_KEYS + j) = v; }
  __device__ uint32_t ver(uint32_t j) const { return at(LCG_VERS + j); }
  __device__ void set_ver(uint32_t j, uint32_t v) const { at(LCG_VERS + j) = v; }
};

// the workgroup's messages, nbytes from g, between global memory and LDS: 16-byte vectors (g is 16-byte aligned: the
// batch buffers are, and LCG_TB * 9 / LCG_TB * 6 are multiples of 16), the tail byte by byte
__device__ static inline void lcg_load(uint8_t *L, const uint8_t *g, uint32_t nbytes, uint32_t t) {
  const uint32_t nv = nbytes / 16;
  for (uint32_t k = t; k < nv; k += LCG_TB) ((uint4 *)L)[k] = ((const uint4 *)g)[k];
  for (uint32_t k = nv * 16 + t; k < nbytes; k += LCG_TB) L[k] = g[k];
}
__device__ static inline void lcg_store(uint8_t *g, const uint8_t *L, uint32_t nbytes, uint32_t t) {
  const uint32_t nv = nbytes / 16;
  for (uint32_t k = t; k < nv; k += LCG_TB) ((uint4 *)g)[k] = ((const uint4 *)L)[k];
  for (uint32_t k = nv * 16 + t; k < nbytes; k += LCG_TB) g[k] = L[k];
}

// WL 0 = lock_fasst, 1 = lock_2pl.  rep != null: consume the replies at rep; out != null: emit the next requests into out;
// init: seed the workers and draw their first transactions (nothing else).
template <int WL>
__global__ void __launch_bounds__(LCG_TB)
k_lock_client(uint32_t *cols, uint32_t n, LcParams P, uint8_t *out, const uint8_t *rep, unsigned long long *st,
              uint32_t first_worker, uint32_t init) {
  constexpr uint32_t MSG = WL == 0 ? sizeof(FasstMsg) : sizeof(TplMsg);
  __shared__ uint4 Lv[LCG_TB * MSG / 16];
  uint8_t *L = (uint8_t *)Lv;
  const uint32_t t = threadIdx.x, lane = t & 63, i = blockIdx.x * LCG_TB + t;
  const bool valid = i < n;
  const uint32_t nbytes = min(LCG_TB, n - blockIdx.x * LCG_TB) * MSG;  // this workgroup's messages
  const size_t base = (size_t)blockIdx.x * LCG_TB * MSG;
  const LcCols s{cols, n, i};
  uint32_t h = 0, ev = 0;
  if (valid) {
    if (init) {
      s.set_rng(0xdeadbeefull + first_worker + i);
      h = lc_new_txn(s, P);
    } else {
      h = cols[i];
    }
  }
  if (rep) {  // (kernel-uniform)
    lcg_load(L, rep + base, nbytes, t);
    __syncthreads();
    if (valid) {
      if (WL == 0) {
        FasstMsg r;
        __builtin_memcpy(&r, L + t * MSG, MSG);
        h = lc_fasst_consume(s, h, P, r.type, r.lid, r.ver, &ev);
      } else {
        h = lc_tpl_consume(s, h, P, L[t * MSG], &ev);  // (the action is byte 0)
      }
    }
    __syncthreads();  // L is rewritten below
  }
  if (out) {
    if (valid) {
      if (WL == 0) {
        uint8_t type;
        const uint32_t j = lc_fasst_req(h, &type);
        const FasstMsg m = {type, s.key(j), 0u};
        __builtin_memcpy(L + t * MSG, &m, MSG);
      } else {
        uint8_t action, type;
        const uint32_t j = lc_tpl_req(h, &action, &type);
        const TplMsg m = {action, s.key(j), type};
        __builtin_memcpy(L + t * MSG, &m, MSG);
      }
    }
    __syncthreads();
    lcg_store(out + base, L, nbytes, t);
  }
  if (valid) cols[i] = h;
  if (rep) {  // statistics: one ballot per counter, one atomic per wave and counter that moved
    const uint32_t c[LCG_NSTAT] = {
        (uint32_t)__popcll(__ballot((ev & LC_EV_COMMIT) != 0)), (uint32_t)__popcll(__ballot((ev & LC_EV_REJECT) != 0)),
        (uint32_t)__popcll(__ballot((ev & LC_EV_ROLLBACK) != 0)),
        (uint32_t)(__popcll(__ballot((ev & LC_EV_PERR_LID) != 0)) + __popcll(__ballot((ev & LC_EV_PERR_TYPE) != 0)))};
    if (lane == 0)
      for (int k = 0; k < LCG_NSTAT; k++)
        if (c[k]) atomicAdd(st + k, (unsigned long long)c[k]);
  }
}

// ------------------------------------------------------------------------------------------------- host side
struct dint_lock_gclient {
  dint_lock_client_config cfg{};
  int device = 0;
  uint32_t msg = 0, ntiles = 0;
  bool awaiting = false;
  bool fuse = true;                      // DINT_LOCK_CLIENT_FUSE=0: consume always in its own kernel
  bool pending = false;                  // a consume deferred into the next emit ...
  hipStream_t pending_stream = nullptr;  // ... which was issued on this stream
  hipStream_t next_stream = nullptr;     // stream of the last dint_lock_gclient_next
  hipEvent_t ev_pending = nullptr;
  uint32_t cur = 0;                      // buffer of the current epoch (the two alternate)
  uint64_t epochs = 0, requests = 0;
  uint32_t *d_cols = nullptr, *d_zipf = nullptr;
  uint8_t *d_batch[2] = {nullptr, nullptr};
  unsigned long long *d_stats = nullptr;
  LcParams P{};
};

namespace {
// rep_set / out_set: buffer whose replies are consumed / into which requests are emitted (-1: none)
void launch(dint_lock_gclient *c, hipStream_t st, int rep_set, int out_set, bool init = false) {
  uint8_t *out = out_set < 0 ? nullptr : c->d_batch[out_set];
  const uint8_t *rep = rep_set < 0 ? nullptr : c->d_batch[rep_set];
  if (c->cfg.workload == DINT_WL_FASST)
    hipLaunchKernelGGL((k_lock_client<0>), dim3(c->ntiles), dim3(LCG_TB), 0, st, c->d_cols, c->cfg.n_workers, c->P, out, rep,
                       c->d_stats, c->cfg.first_worker, (uint32_t)init);
  else
    hipLaunchKernelGGL((k_lock_client<1>), dim3(c->ntiles), dim3(LCG_TB), 0, st, c->d_cols, c->cfg.n_workers, c->P, out, rep,
                       c->d_stats, c->cfg.first_worker, (uint32_t)init);
}
// a consume deferred into the next emit runs now, on the stream it was promised on
int flush_pending(dint_lock_gclient *c) {
  if (!c->pending) return 0;
  launch(c, c->pending_stream, (int)c->cur, -1);
  c->pending = false;
  return hipGetLastError() == hipSuccess ? 0 : DINT_EHIP;
}
}  // namespace

extern "C" {

int dint_lock_gclient_create(const dint_lock_client_config *cfg, int32_t device, dint_lock_gclient_t **out) {
  if (!cfg || !out || (cfg->workload != DINT_WL_FASST && cfg->workload != DINT_WL_2PL)) return DINT_EINVAL;
  dint_fasst_client_config fc;
  memcpy(&fc, cfg, sizeof fc);
  LcParams P{};
  ZipfTable zipf;
  try {
    if (int rc = dint_lock_client_params(&fc, &P, &zipf)) return rc;  // (the config is checked before any device call)
  } catch (const std::bad_alloc &) {
    return DINT_ENOMEM;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return DINT_ENODEV;
  if (device < 0 && hipGetDevice(&device) != hipSuccess) return DINT_ENODEV;
  if (device >= ndev || hipSetDevice(device) != hipSuccess) return DINT_ENODEV;
  dint_lock_gclient *c = new (std::nothrow) dint_lock_gclient();
  if (!c) return DINT_ENOMEM;
  c->cfg = *cfg;
  c->device = device;
  c->P = P;
  c->msg = cfg->workload == DINT_WL_FASST ? sizeof(FasstMsg) : sizeof(TplMsg);
  c->ntiles = (cfg->n_workers + LCG_TB - 1) / LCG_TB;
  if (getenv("DINT_LOCK_CLIENT_FUSE")) c->fuse = atoi(getenv("DINT_LOCK_CLIENT_FUSE")) != 0;
  const size_t ncol = cfg->workload == DINT_WL_FASST ? LCG_VERS + LC_MAXK : LCG_KEYS + LC_MAXK;
  const size_t cbytes = ncol * cfg->n_workers * sizeof(uint32_t);
  int rc = 0;
  if (hipMalloc((void **)&c->d_cols, cbytes) != hipSuccess || hipMalloc((void **)&c->d_stats, LCG_NSTAT * 8) != hipSuccess)
    rc = DINT_ENOMEM;
  for (int b = 0; b < 2 && !rc; b++)
    if (hipMalloc((void **)&c->d_batch[b], (size_t)cfg->n_workers * c->msg + 64) != hipSuccess) rc = DINT_ENOMEM;
  if (!rc && cfg->key_dist == 1) {
    if (hipMalloc((void **)&c->d_zipf, zipf.cdf.size() * 4) != hipSuccess) rc = DINT_ENOMEM;
    else if (hipMemcpy(c->d_zipf, zipf.cdf.data(), zipf.cdf.size() * 4, hipMemcpyHostToDevice) != hipSuccess) rc = DINT_EHIP;
    c->P.zipf_cdf = c->d_zipf;
  }
  if (!rc && hipEventCreateWithFlags(&c->ev_pending, hipEventDisableTiming) != hipSuccess) rc = DINT_EHIP;
  if (!rc && (hipMemset(c->d_cols, 0, cbytes) != hipSuccess || hipMemset(c->d_stats, 0, LCG_NSTAT * 8) != hipSuccess ||
              hipMemset(c->d_batch[0], 0, (size_t)cfg->n_workers * c->msg + 64) != hipSuccess ||
              hipMemset(c->d_batch[1], 0, (size_t)cfg->n_workers * c->msg + 64) != hipSuccess ||
              hipDeviceSynchronize() != hipSuccess))
    rc = DINT_EHIP;
  if (!rc) {  // every worker draws its first transaction
    launch(c, nullptr, -1, -1, true);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = DINT_EHIP;
  }
  if (rc) {
    dint_lock_gclient_destroy(c);
    return rc;
  }
  *out = c;
  return 0;
}

void dint_lock_gclient_destroy(dint_lock_gclient_t *c) {
  if (!c) return;
  hipSetDevice(c->device);
  hipDeviceSynchronize();
  hipFree(c->d_cols);
  hipFree(c->d_zipf);
  hipFree(c->d_batch[0]);
  hipFree(c->d_batch[1]);
  hipFree(c->d_stats);
  if (c->ev_pending) hipEventDestroy(c->ev_pending);
  delete c;
}

int dint_lock_gclient_next(dint_lock_gclient_t *c, void *stream) {
  if (!c) return DINT_EINVAL;
  if (c->awaiting) return DINT_ESTATE;
  if (hipSetDevice(c->device) != hipSuccess) return DINT_EHIP;
  hipStream_t st = (hipStream_t)stream;
  bool fused = false;
  if (c->pending) {
    if (st == c->pending_stream) {
      fused = true;  // the replies are taken by the emit kernel itself
      c->pending = false;
    } else {  // consume was promised on another stream: run it there, and this stream behind it
      if (int rc = flush_pending(c)) return rc;
      if (hipEventRecord(c->ev_pending, c->pending_stream) != hipSuccess || hipStreamWaitEvent(st, c->ev_pending, 0) != hipSuccess)
        return DINT_EHIP;
    }
  }
  const uint32_t o = c->cur;
  c->cur ^= 1u;
  launch(c, st, fused ? (int)o : -1, (int)c->cur);
  if (hipGetLastError() != hipSuccess) return DINT_EHIP;
  c->next_stream = st;
  c->awaiting = true;
  c->epochs++;
  c->requests += c->cfg.n_workers;
  return 0;
}

// The replies are in place in the current batch.  Issued on the stream of the last dint_lock_gclient_next (the closed loop),
// the consume is deferred into the next emit kernel; the stream must then still exist at the next dint_lock_gclient_next.
// On any other stream (or with DINT_LOCK_CLIENT_FUSE=0) it runs now, in a kernel of its own.
int dint_lock_gclient_consume(dint_lock_gclient_t *c, void *stream) {
  if (!c) return DINT_EINVAL;
  if (!c->awaiting) return DINT_ESTATE;
  if (hipSetDevice(c->device) != hipSuccess) return DINT_EHIP;
  hipStream_t st = (hipStream_t)stream;
  if (c->fuse && st == c->next_stream) {
    c->pending = true;
    c->pending_stream = st;
  } else {
    launch(c, st, (int)c->cur, -1);
    if (hipGetLastError() != hipSuccess) return DINT_EHIP;
  }
  c->awaiting = false;
  return 0;
}

// the CURRENT epoch's batch: the two buffers alternate, ask again after every dint_lock_gclient_next
void *dint_lock_gclient_batch(dint_lock_gclient_t *c) { return c ? c->d_batch[c->cur] : nullptr; }

int dint_lock_gclient_read_batch(dint_lock_gclient_t *c, void *host) {
  if (!c || !host) return DINT_EINVAL;
  if (hipSetDevice(c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return DINT_EHIP;
  if (hipMemcpy(host, c->d_batch[c->cur], (size_t)c->cfg.n_workers * c->msg, hipMemcpyDeviceToHost) != hipSuccess) return DINT_EHIP;
  return 0;
}

int dint_lock_gclient_get_stats(dint_lock_gclient_t *c, dint_fasst_client_stats *out) {
  if (!c || !out) return DINT_EINVAL;
  if (hipSetDevice(c->device) != hipSuccess) return DINT_EHIP;
  if (int rc = flush_pending(c)) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return DINT_EHIP;
  unsigned long long s[LCG_NSTAT];
  if (hipMemcpy(s, c->d_stats, sizeof s, hipMemcpyDeviceToHost) != hipSuccess) return DINT_EHIP;
  memset(out, 0, sizeof *out);
  out->requests = c->requests;
  out->epochs = c->epochs;
  out->committed = s[0];
  out->rejects = s[1];
  out->rollbacks = s[2];
  out->protocol_errors = s[3];
  return 0;
}

}  // extern "C"
