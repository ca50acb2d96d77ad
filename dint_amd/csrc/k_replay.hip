// k_replay.hip -- a drained log replayed into a replica without leaving the GPU (include/dint_abi.h
// dint_log_apply_device, driven by engine.hip).
//
// dint_amd/recovery.py apply_log as device code.  Per chunk of at most one pass of records (tatp):
//
//   k_replay_keys      one lane per record: the row word (log_replay.h lr_row: table above the key) and the record's index
//   radix sort         (row, index) pairs, stable: the records of a row become neighbours and keep log order
//   k_replay_probe     the first record of every row of the chunk asks the replica whether the row exists: one READ, compacted
//                      into the probe batch (a workgroup takes its READs' places with one atomic; their order is free: a READ
//                      changes nothing).  The replica answers in place through its ordinary pass (a one-segment view whose
//                      live count is the device word the kernel counted in: the host never learns the number of rows)
//   k_replay_classify  sorted position p: the row exists before record idx[p] if the previous record of the row was no
//                      delete -- or, for the first of a row, if the probe said GRANT_READ; the request type goes to types[i]
//   k_replay_emit      one lane per record, log order: the 55-byte COMMIT_BCK / INSERT_BCK / DELETE_BCK message
//   (the replica answers the batch in place)
//   k_replay_count     the acks by type: one ballot per counter, one atomic per wave and counter that moved
//
// smallbank has no inserts or deletes: emit (23-byte COMMIT_BCK, val = the record's first 8 bytes) and count only.
// Messages are unaligned (55 / 23 bytes): a workgroup builds its messages in LDS and stores them as 16-byte vectors, as
// k_lock_client.hip does; 256 messages of either size are a whole number of vectors.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <numeric>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "../../include/dint_abi.h"
#include "../../include/dint_driver.h"
#include "dint_kernels.h"
#include "log_replay.h"

#define RP_TB 256u  // records per workgroup

static_assert((RP_TB * sizeof(LrTatpMsg)) % 16 == 0 && (RP_TB * sizeof(LrSbMsg)) % 16 == 0, "a workgroup's messages are whole vectors");

// the two vectors of a record that hold everything but val[8..40): {key, val[0..8)} and {val[40 - 48 ..], ver, is_del, table}
__device__ static inline uint64_t rp_key(const uint4 &v0) { return (uint64_t)v0.x | (uint64_t)v0.y << 32; }
__device__ static inline uint8_t rp_is_del(const uint4 &v3) { return (uint8_t)(v3.y & 0xFF); }
__device__ static inline uint8_t rp_table(const uint4 &v3) { return (uint8_t)((v3.y >> 8) & 0xFF); }
static_assert(offsetof(LrRecord, ver) == 48 && offsetof(LrRecord, is_del) == 52 && offsetof(LrRecord, table) == 53, "record layout");

__global__ void __launch_bounds__(RP_TB)
k_replay_keys(const uint4 *rec, uint32_t m, uint64_t *row, uint32_t *idx, uint32_t *probe_n) {
  const uint32_t i = blockIdx.x * RP_TB + threadIdx.x;
  if (i == 0) *probe_n = 0;  // (counted up by k_replay_probe, two launches on)
  if (i >= m) return;
  const uint4 v0 = rec[(size_t)i * 4], v3 = rec[(size_t)i * 4 + 3];
  row[i] = lr_row(rp_table(v3), rp_key(v0));
  idx[i] = i;
}

// nbytes of the workgroup's LDS image, starting at byte `a` of it, to g + a (g 16-byte aligned): whole vectors where the
// image covers them, single bytes at the two ends
__device__ static inline void rp_store(uint8_t *g, const uint8_t *L, uint32_t a, uint32_t nbytes, uint32_t t) {
  const uint32_t end = a + nbytes, v0 = (a + 15) / 16, v1 = end / 16;
  if (v0 >= v1) {  // (fewer bytes than one aligned vector)
    for (uint32_t k = a + t; k < end; k += RP_TB) g[k] = L[k];
    return;
  }
  for (uint32_t k = v0 + t; k < v1; k += RP_TB) ((uint4 *)g)[k] = ((const uint4 *)L)[k];
  for (uint32_t k = a + t; k < v0 * 16; k += RP_TB) g[k] = L[k];
  for (uint32_t k = v1 * 16 + t; k < end; k += RP_TB) g[k] = L[k];
}

__global__ void __launch_bounds__(RP_TB)
k_replay_probe(const uint8_t *rec, const uint64_t *row, const uint32_t *idx, uint32_t m, uint32_t *slot, uint8_t *probe,
               uint32_t *probe_n) {
  constexpr uint32_t MSG = sizeof(LrTatpMsg);
  __shared__ uint4 Lv[(16 + RP_TB * MSG + 15) / 16];
  __shared__ uint32_t wave_n[RP_TB / 64], base_s;
  uint8_t *L = (uint8_t *)Lv;
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6, p = blockIdx.x * RP_TB + t;
  const bool head = p < m && (p == 0 || row[p - 1] != row[p]);
  const unsigned long long b = __ballot(head);
  if (lane == 0) wave_n[w] = (uint32_t)__popcll(b);
  __syncthreads();
  uint32_t before = 0, total = 0;
  for (uint32_t k = 0; k < RP_TB / 64; k++) {
    if (k < w) before += wave_n[k];
    total += wave_n[k];
  }
  if (t == 0) base_s = total ? atomicAdd(probe_n, total) : 0u;  // (at most m READs in all: the batch holds max(m, 2))
  __syncthreads();
  if (total == 0) return;  // (workgroup-uniform)
  const uint32_t base = base_s;
  const uint32_t a = (uint32_t)(((size_t)base * MSG) & 15);  // the image sits in LDS at the batch's own 16-byte phase
  if (head) {
    const uint32_t r = before + (uint32_t)__popcll(b & ((1ull << lane) - 1));
    const uint8_t *rc = rec + (size_t)idx[p] * sizeof(LrRecord);
    LrTatpMsg q;
    __builtin_memset(&q, 0, MSG);
    q.type = LR_T_READ;
    q.table = rc[offsetof(LrRecord, table)];
    q.key = *(const uint64_t *)rc;
    __builtin_memcpy(L + a + r * MSG, &q, MSG);
    slot[p] = base + r;
  }
  __syncthreads();
  rp_store(probe + (((size_t)base * MSG) & ~(size_t)15), L, a, total * MSG, t);
}

__global__ void __launch_bounds__(RP_TB)
k_replay_classify(const uint8_t *rec, const uint64_t *row, const uint32_t *idx, const uint32_t *slot, const uint8_t *probe,
                  uint32_t m, uint8_t *types) {
  const uint32_t p = blockIdx.x * RP_TB + threadIdx.x;
  if (p >= m) return;
  const uint32_t i = idx[p];
  const bool is_del = rec[(size_t)i * sizeof(LrRecord) + offsetof(LrRecord, is_del)] != 0;
  bool exists;
  if (p == 0 || row[p - 1] != row[p])
    exists = probe[(size_t)slot[p] * sizeof(LrTatpMsg) + offsetof(LrTatpMsg, type)] == LR_T_GRANT_READ;
  else
    exists = lr_exists_after(rec[(size_t)idx[p - 1] * sizeof(LrRecord) + offsetof(LrRecord, is_del)]);
  types[i] = lr_tatp_type(is_del, exists);
}

// SB = false: tatp, the type chosen by k_replay_classify; true: smallbank COMMIT_BCK
template <bool SB>
__global__ void __launch_bounds__(RP_TB)
k_replay_emit(const uint4 *rec, const uint8_t *types, uint32_t m, uint8_t *msgs) {
  constexpr uint32_t MSG = SB ? sizeof(LrSbMsg) : sizeof(LrTatpMsg);
  __shared__ uint4 Lv[RP_TB * MSG / 16];
  uint8_t *L = (uint8_t *)Lv;
  const uint32_t t = threadIdx.x, i = blockIdx.x * RP_TB + t;
  const uint32_t nbytes = min(RP_TB, m - blockIdx.x * RP_TB) * MSG;  // this workgroup's messages (the grid covers m exactly)
  if (i < m) {
    uint4 v[4];
    for (int k = 0; k < 4; k++) v[k] = rec[(size_t)i * 4 + k];
    LrRecord r;
    __builtin_memcpy(&r, v, sizeof r);
    if (SB) {
      LrSbMsg q;
      q.ord = 0; q.type = LR_S_COMMIT_BCK; q.table = r.table; q.key = r.key; q.ver = r.ver;
      __builtin_memcpy(q.val, r.val, sizeof q.val);
      __builtin_memcpy(L + t * MSG, &q, MSG);
    } else {
      LrTatpMsg q;
      q.ord = 0; q.type = types[i]; q.table = r.table; q.key = r.key; q.ver = r.ver;
      __builtin_memcpy(q.val, r.val, sizeof q.val);
      __builtin_memcpy(L + t * MSG, &q, MSG);
    }
  }
  __syncthreads();
  rp_store(msgs + (size_t)blockIdx.x * RP_TB * MSG, L, 0, nbytes, t);
}

// replies in place in msgs: acks of type t0 / t1 / t2 into counts[0..2]
__global__ void __launch_bounds__(RP_TB)
k_replay_count(const uint8_t *msgs, uint32_t m, uint32_t msg, uint8_t t0, uint8_t t1, uint8_t t2, unsigned long long *counts) {
  const uint32_t i = blockIdx.x * RP_TB + threadIdx.x;
  const uint32_t ty = i < m ? msgs[(size_t)i * msg + 1] : 0xFFFFFFFFu;  // (the type is byte 1 of both messages)
  const uint32_t c[3] = {(uint32_t)__popcll(__ballot(ty == t0)), (uint32_t)__popcll(__ballot(ty == t1)),
                         (uint32_t)__popcll(__ballot(ty == t2))};
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < 3; k++)
      if (c[k]) atomicAdd(counts + k, (unsigned long long)c[k]);
}

// ------------------------------------------------------------------------------------------------- host side
static inline uint32_t rp_grid(uint32_t m) { return (m + RP_TB - 1) / RP_TB; }

int64_t dint_replay_sort_bytes(uint32_t m, hipStream_t st) {
  size_t bytes = 0;
  if (rocprim::radix_sort_pairs(nullptr, bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr,
                                (uint32_t *)nullptr, (size_t)m, 0u, 64u, st) != hipSuccess)
    return -1;
  return (int64_t)bytes;
}

bool dint_launch_replay_group(const void *d_rec, uint32_t m, dint_replay_scratch s, hipStream_t st) {
  if (m == 0) return true;
  hipLaunchKernelGGL(k_replay_keys, dim3(rp_grid(m)), dim3(RP_TB), 0, st, (const uint4 *)d_rec, m, s.row_in, s.idx_in, s.probe_n);
  size_t bytes = s.sort_tmp_bytes;
  if (rocprim::radix_sort_pairs(s.sort_tmp, bytes, (const uint64_t *)s.row_in, s.row_out, (const uint32_t *)s.idx_in, s.idx_out,
                                (size_t)m, 0u, 64u, st) != hipSuccess)
    return false;
  hipLaunchKernelGGL(k_replay_probe, dim3(rp_grid(m)), dim3(RP_TB), 0, st, (const uint8_t *)d_rec, s.row_out, s.idx_out, m, s.slot,
                     s.probe, s.probe_n);
  return true;
}

void dint_launch_replay_emit(const void *d_rec, uint32_t m, dint_replay_scratch s, hipStream_t st) {
  if (m == 0) return;
  hipLaunchKernelGGL(k_replay_classify, dim3(rp_grid(m)), dim3(RP_TB), 0, st, (const uint8_t *)d_rec, s.row_out, s.idx_out, s.slot,
                     s.probe, m, s.types);
  hipLaunchKernelGGL((k_replay_emit<false>), dim3(rp_grid(m)), dim3(RP_TB), 0, st, (const uint4 *)d_rec, s.types, m, s.msgs);
}

void dint_launch_replay_emit_sb(const void *d_rec, uint32_t m, dint_replay_scratch s, hipStream_t st) {
  if (m == 0) return;
  hipLaunchKernelGGL((k_replay_emit<true>), dim3(rp_grid(m)), dim3(RP_TB), 0, st, (const uint4 *)d_rec, (const uint8_t *)nullptr, m, s.msgs);
}

void dint_launch_replay_count(uint32_t workload, uint32_t m, dint_replay_scratch s, hipStream_t st) {
  if (m == 0) return;
  if (workload == DINT_WL_SMALLBANK)  // (0xFE / 0xFF: no reply carries them)
    hipLaunchKernelGGL(k_replay_count, dim3(rp_grid(m)), dim3(RP_TB), 0, st, s.msgs, m, (uint32_t)sizeof(LrSbMsg),
                       (uint8_t)LR_S_COMMIT_BCK_ACK, (uint8_t)0xFE, (uint8_t)0xFF, s.counts);
  else
    hipLaunchKernelGGL(k_replay_count, dim3(rp_grid(m)), dim3(RP_TB), 0, st, s.msgs, m, (uint32_t)sizeof(LrTatpMsg),
                       (uint8_t)LR_T_COMMIT_BCK_ACK, (uint8_t)LR_T_INSERT_BCK_ACK, (uint8_t)LR_T_DELETE_BCK_ACK, s.counts);
}

// the rule of k_replay_classify on the host (include/dint_driver.h): the same grouping -- a stable sort of (row, index) --
// and the same log_replay.h functions
extern "C" int dint_log_classify_host(const void *records, uint64_t n, const uint8_t *exists0, uint8_t *types_out) {
  if (n && (!records || !exists0 || !types_out)) return DINT_EINVAL;
  if (n > 0xFFFFFFFFull) return DINT_EINVAL;
  const LrRecord *rec = (const LrRecord *)records;
  try {
    std::vector<uint64_t> row(n);
    std::vector<uint32_t> idx(n);
    for (uint64_t i = 0; i < n; i++) row[i] = lr_row(rec[i].table, rec[i].key);
    std::iota(idx.begin(), idx.end(), 0u);
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return row[x] < row[y]; });
    for (uint64_t p = 0; p < n; p++) {
      const uint32_t i = idx[p];
      const bool head = p == 0 || row[idx[p - 1]] != row[i];
      const bool exists = head ? exists0[i] != 0 : lr_exists_after(rec[idx[p - 1]].is_del);
      types_out[i] = lr_tatp_type(rec[i].is_del != 0, exists);
    }
  } catch (const std::bad_alloc &) {
    return DINT_ENOMEM;
  }
  return 0;
}
