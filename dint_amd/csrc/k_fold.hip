// k_fold.hip -- a chunk of a drained log folded per row on the GPU and handed to the state repair (include/dint_abi.h
// dint_log_apply_folded_device, driven by engine.hip; the rule is log_fold.h's, which the host form at the end of this file shares).
//
// Per chunk of at most one pass of records:
//
//   k_fold_keys        one lane per record: the row word (log_replay.h lr_row), the record's index, its place word (table, bucket)
//   radix sort x 2     order (table, bucket, key, log index).  The composite key would be 3 + 32 + 64 bits, more than a radix sort
//                      key holds, so: k_replay.hip's stable (row, index) sort over 64 bits, then a stable sort on the 35 bits of the
//                      place word (k_fold_place gathers it into sorted order in between)
//   k_fold_gather      key and is_del of the record at sorted position p, and "p + 1 if it is a delete" for the max-scan
//   k_fold_heads       the first position of every row; an inclusive sum gives every position its row, an inclusive max the
//                      position of the last delete so far (log_fold.h: why the plain maximum is the segmented one here)
//   k_fold_rows        the row list: row r starts at row_start[r]
//   k_fold_probe       one lane per row walks the replica's chain once (state_dev.h sd_bucket, state_image.h si_chain_walk), counts
//                      the slots that hold the key and keeps the version of the first
//   k_fold_bucket      one lane per bucket of the row list ORs "occ >= 2" over the bucket's rows and stamps it on them
//   k_fold_net         one lane per row: the row's last position and last delete -> its net effect (lf_fold); never a lane
//                      looping over its row's records
//   k_fold_emit        the rows that have one, compacted by an exclusive sum (sorted order is ascending (table, bucket) already),
//                      as 64-byte repair records; the value moves in 16-byte vectors
//   k_fold_count       one lane per sorted position: the record as a backup operation, counted by ballot -- one atomic per wave
//                      and counter that moved -- and defer[log index]
//   k_fold_defer       the deferred records, stable-compacted in log order (an exclusive sum), 4 lanes per record
//   k_fold_totals      the chunk's three words for the host: deferred records, repair records, rows
//   k_fold_rotate      in front of the repair: the pool's pend lists rotated into its free lists, as a hot-path pass would
// A record is read through the two vectors that hold everything but val[8..40), as k_replay.hip reads it.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <numeric>
#include <unordered_map>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "../../include/dint_abi.h"
#include "../../include/dint_driver.h"
#include "dint_kernels.h"
#include "dint_kv.h"
#include "log_fold.h"
#include "state_dev.h"

#define FD_TB SD_TB  // threads per workgroup, every kernel here

__device__ static inline uint64_t fd_key(const uint4 &v0) { return (uint64_t)v0.x | (uint64_t)v0.y << 32; }
__device__ static inline uint8_t fd_is_del(const uint4 &v3) { return (uint8_t)(v3.y & 0xFF); }
__device__ static inline uint8_t fd_table(const uint4 &v3) { return (uint8_t)((v3.y >> 8) & 0xFF); }
static_assert(offsetof(LrRecord, ver) == 48 && offsetof(LrRecord, is_del) == 52 && offsetof(LrRecord, table) == 53, "record layout");

__global__ void __launch_bounds__(FD_TB)
k_fold_keys(const uint4 *__restrict__ rec, uint32_t m, const kv_dev *__restrict__ kv, uint64_t *row, uint32_t *idx, uint64_t *place) {
  const uint32_t i = blockIdx.x * FD_TB + threadIdx.x;
  if (i >= m) return;
  const uint4 v0 = rec[(size_t)i * 4], v3 = rec[(size_t)i * 4 + 3];
  const uint32_t table = fd_table(v3);
  const uint64_t key = fd_key(v0);
  row[i] = lr_row((uint8_t)table, key);
  idx[i] = i;
  // (the LOCAL bucket: k_fold_probe indexes this engine's own table, and the repair records leave in the shard's order.  A record of
  // another shard never gets here -- the call's check pass refused the list -- and would be set aside like one of a bad table)
  const uint64_t b = table < kv->n_tables ? rr_local(key, table, kv->mod, kv->shard_index, kv->shard_count) : SR_FOREIGN;
  place[i] = b != SR_FOREIGN ? lf_place(table, b) : lf_place(LF_BAD_TABLE, 0);
}

__global__ void __launch_bounds__(FD_TB)
k_fold_place(const uint64_t *__restrict__ place, const uint32_t *__restrict__ idx, uint32_t m, uint64_t *out) {
  const uint32_t p = blockIdx.x * FD_TB + threadIdx.x;
  if (p < m) out[p] = place[idx[p]];
}

template <bool SB>
__global__ void __launch_bounds__(FD_TB)
k_fold_gather(const uint4 *__restrict__ rec, const uint32_t *__restrict__ idx, uint32_t m, uint64_t *key_s, uint8_t *del_s,
              uint32_t *delpos) {
  const uint32_t p = blockIdx.x * FD_TB + threadIdx.x;
  if (p >= m) return;
  const size_t i = idx[p];
  key_s[p] = fd_key(rec[i * 4]);
  const uint8_t del = SB ? (uint8_t)0 : (uint8_t)(fd_is_del(rec[i * 4 + 3]) != 0);
  del_s[p] = del;
  delpos[p] = del ? p + 1u : 0u;
}

__device__ static inline bool fd_head(const uint64_t *place_s, const uint64_t *key_s, uint32_t p) {
  return p == 0 || place_s[p - 1] != place_s[p] || key_s[p - 1] != key_s[p];
}

__global__ void __launch_bounds__(FD_TB)
k_fold_heads(const uint64_t *__restrict__ place_s, const uint64_t *__restrict__ key_s, uint32_t m, uint32_t *flag) {
  const uint32_t p = blockIdx.x * FD_TB + threadIdx.x;
  if (p < m) flag[p] = fd_head(place_s, key_s, p) ? 1u : 0u;
}

// words[2] = the rows of the chunk
__global__ void __launch_bounds__(FD_TB)
k_fold_rows(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ rowid, uint32_t m, uint32_t *row_start, uint32_t *words) {
  const uint32_t p = blockIdx.x * FD_TB + threadIdx.x;
  if (p >= m) return;
  if (flag[p]) row_start[rowid[p] - 1u] = p;  // (rowid[p] <= p + 1 <= m)
  if (p == m - 1) {
    row_start[rowid[p]] = m;  // (row_start holds m + 1 words)
    words[2] = rowid[p];
  }
}

__global__ void __launch_bounds__(FD_TB)
k_fold_probe(const kv_dev *__restrict__ kv, const uint64_t *__restrict__ place_s, const uint64_t *__restrict__ key_s,
             const uint32_t *__restrict__ row_start, const uint32_t *__restrict__ words, uint32_t *row_occ, uint32_t *row_v0) {
  const uint32_t r = blockIdx.x * FD_TB + threadIdx.x;
  if (r >= words[2]) return;
  const uint32_t p = row_start[r];
  const uint64_t place = place_s[p], key = key_s[p];
  const uint32_t table = lf_place_table(place);
  uint32_t occ = 0, v0 = 0;
  if (table >= kv->n_tables) {
    occ = 2;  // (a table the workload has not: the serial replay answers such a record)
  } else {
    const kv_tab t = kv->tab[table];
    const uint64_t b = lf_place_bucket(place);  // (< n_local: the local bucket k_fold_keys placed it at)
    const sd_bucket ch = sd_bucket_at(t, b);
    const bool ok = si_chain_walk(ch.head(), ch, [&](uint32_t, uint32_t link, uint32_t validw) {
      if (!validw) return true;
      uint64_t k[4];
      ch.keys(link, k);
#pragma unroll
      for (uint32_t s = 0; s < 4; s++)
        if (((validw >> (8 * s)) & 0xFFu) && k[s] == key) {
          if (occ == 0) v0 = KV_LD(uint32_t, kv_entry_ptr(t, b, link) + offsetof(kv_hdr, ver) + 4 * s);
          occ++;
        }
      return true;
    });
    if (!ok) occ = 2;  // (a chain that cannot be walked to its end: nothing is concluded from it)
  }
  row_occ[r] = occ;
  row_v0[r] = v0;
}

// counts[7] += the deferred buckets
__global__ void __launch_bounds__(FD_TB)
k_fold_bucket(const uint64_t *__restrict__ place_s, const uint32_t *__restrict__ row_start, const uint32_t *__restrict__ words,
              const uint32_t *__restrict__ row_occ, uint8_t *row_defer, unsigned long long *counts) {
  const uint32_t r = blockIdx.x * FD_TB + threadIdx.x, n_rows = words[2];
  bool deferred = false;
  if (r < n_rows) {
    const uint64_t place = place_s[row_start[r]];
    if (r == 0 || place_s[row_start[r - 1]] != place) {  // the first row of a bucket owns its few rows
      uint32_t e = r;
      for (; e < n_rows && place_s[row_start[e]] == place; e++) deferred |= lf_defers(row_occ[e]);
      for (uint32_t k = r; k < e; k++) row_defer[k] = deferred;
    }
  }
  const uint32_t c = (uint32_t)__popcll(__ballot(deferred));
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(counts + 7, (unsigned long long)c);
}

// every r < m: has[r] = row r emits a repair record (0 for r beyond the rows)
template <bool SB>
__global__ void __launch_bounds__(FD_TB)
k_fold_net(uint32_t m, const uint32_t *__restrict__ row_start, const uint32_t *__restrict__ words, const uint32_t *__restrict__ lastdel,
           const uint32_t *__restrict__ row_occ, const uint32_t *__restrict__ row_v0, const uint8_t *__restrict__ row_defer,
           uint32_t *row_kind, uint32_t *row_ver, uint32_t *has) {
  const uint32_t r = blockIdx.x * FD_TB + threadIdx.x;
  if (r >= m) return;
  uint32_t h = 0;
  if (r < words[2]) {
    const uint32_t s = row_start[r], q = row_start[r + 1] - 1u;
    const uint32_t d = SB ? 0u : lf_last_delete(lastdel[q], s);
    const lf_net net = lf_fold(SB, row_occ[r], row_v0[r], q - s + 1u, d);
    row_kind[r] = net.kind;
    row_ver[r] = net.ver;
    h = !row_defer[r] && net.kind != LF_NONE;
  }
  has[r] = h;
}

template <bool SB>
__global__ void __launch_bounds__(FD_TB)
k_fold_emit(const uint4 *__restrict__ rec, const uint32_t *__restrict__ idx_s, const uint64_t *__restrict__ place_s,
            const uint64_t *__restrict__ key_s, const uint32_t *__restrict__ row_start, const uint32_t *__restrict__ words,
            const uint32_t *__restrict__ row_kind, const uint32_t *__restrict__ row_ver, const uint32_t *__restrict__ has,
            const uint32_t *__restrict__ epos, uint4 *out) {
  const uint32_t r = blockIdx.x * FD_TB + threadIdx.x;
  if (r >= words[2] || !has[r]) return;
  const uint32_t s = row_start[r], q = row_start[r + 1] - 1u;
  const lf_net net = {row_kind[r], row_ver[r]};
  uint32_t last[16], w[16];
  if (net.kind == LF_PUT) {
    const uint4 *src = rec + (size_t)idx_s[q] * 4;
    const uint4 a = src[0], b = src[1], c = src[2];
    last[0] = a.x; last[1] = a.y; last[2] = a.z; last[3] = a.w;
    last[4] = b.x; last[5] = b.y; last[6] = b.z; last[7] = b.w;
    last[8] = c.x; last[9] = c.y; last[10] = c.z; last[11] = c.w;
    last[12] = last[13] = last[14] = last[15] = 0;
  } else {
    for (int i = 0; i < 16; i++) last[i] = 0;
  }
  lf_record(w, SB, net, key_s[s], lf_place_table(place_s[s]), last);
  uint4 *o = out + (size_t)epos[r] * 4;  // (epos[r] < rows <= m <= the scratch's records)
#pragma unroll
  for (int k = 0; k < 4; k++) o[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}

// counts[0..2] / [3..5] += the folded / deferred records as commits, inserts, deletes; dflag[log index] = deferred
template <bool SB>
__global__ void __launch_bounds__(FD_TB)
k_fold_count(uint32_t m, const uint32_t *__restrict__ idx_s, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ rowid,
             const uint8_t *__restrict__ del_s, const uint32_t *__restrict__ row_occ, const uint8_t *__restrict__ row_defer,
             uint32_t *dflag, unsigned long long *counts) {
  const uint32_t p = blockIdx.x * FD_TB + threadIdx.x;
  uint32_t which = 0xFFFFFFFFu;
  if (p < m) {
    const uint32_t r = rowid[p] - 1u;
    const bool first = flag[p] != 0;
    const uint32_t deferred = row_defer[r] ? 1u : 0u;
    which = 3u * deferred + lf_kind(SB, del_s[p], first, row_occ[r], first ? (uint8_t)0 : del_s[p - 1]);
    dflag[idx_s[p]] = deferred;
  }
#pragma unroll
  for (uint32_t k = 0; k < 6; k++) {
    const uint32_t c = (uint32_t)__popcll(__ballot(which == k));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(counts + k, (unsigned long long)c);
  }
}

// 4 lanes per record, a 16-byte vector each
__global__ void __launch_bounds__(FD_TB)
k_fold_defer(const uint4 *__restrict__ rec, uint32_t m, const uint32_t *__restrict__ dflag, const uint32_t *__restrict__ dpos, uint4 *out) {
  const uint32_t g = blockIdx.x * FD_TB + threadIdx.x, i = g >> 2, v = g & 3u;
  if (i >= m || !dflag[i]) return;
  out[(size_t)dpos[i] * 4 + v] = rec[(size_t)i * 4 + v];  // (dpos[i] <= i)
}

__global__ void k_fold_totals(uint32_t m, const uint32_t *__restrict__ dflag, const uint32_t *__restrict__ dpos,
                              const uint32_t *__restrict__ has, const uint32_t *__restrict__ epos, uint32_t *words,
                              unsigned long long *counts) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const uint32_t n_def = dpos[m - 1] + dflag[m - 1], n_emit = epos[m - 1] + has[m - 1];
  words[0] = n_def;
  words[1] = n_emit;
  counts[6] += n_def;
  counts[8] += words[2];
  counts[9] += n_emit;
}

// device-scope RMWs on the pool words, as the kv kernels (k_kv_dev.h kv_dev_mem) and k_state.hip
struct fd_dev_mem {
  __device__ static inline uint32_t fetch_add(uint32_t *p, uint32_t v) { return atomicAdd(p, v); }
  __device__ static inline uint32_t load32(uint32_t *p) { return atomicAdd(p, 0u); }
  __device__ static inline void store32(uint32_t *p, uint32_t v) { atomicExch(p, v); }
  __device__ static inline unsigned long long load64(unsigned long long *p) { return atomicAdd(p, 0ull); }
  __device__ static inline bool cas64(unsigned long long *p, unsigned long long exp, unsigned long long des) {
    return atomicCAS(p, exp, des) == exp;
  }
};
// The pool's pass boundary for a replica that sees no hot-path pass: overflow entries the repair emptied sit on a pend list until
// a partition kernel rotates it (dint_kv_core.h kv_pool_rotate), and a fold that defers nothing launches none.  One thread per
// list, both pend sets: this kernel runs alone on the engine's stream, behind every kernel that pushed to either set and in front
// of the repair that pops, so what it moves was freed a launch ago at least -- the discipline of the partition's own rotation.
__global__ void __launch_bounds__(KV_NLISTS) k_fold_rotate(const kv_dev *__restrict__ kv) {
  const uint32_t lst = threadIdx.x;
  for (uint32_t k = 0; k < kv->n_tables; k++) {
    kv_pool_rotate<fd_dev_mem>(kv->tab[k], lst, 0);
    kv_pool_rotate<fd_dev_mem>(kv->tab[k], lst, KV_NLISTS);  // (only into a list that is still empty)
  }
}

__global__ void k_fold_harvest(const unsigned long long *__restrict__ w, unsigned long long *counts) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int k = 0; k < 4; k++) counts[10 + k] += w[1 + k];
  counts[14] |= w[0];
}

// ------------------------------------------------------------------------------------------------- host side
static inline uint32_t fd_grid(uint64_t n) { return (uint32_t)((n + FD_TB - 1) / FD_TB); }

int64_t dint_fold_tmp_bytes(uint32_t m, hipStream_t st) {
  size_t a = 0, b = 0, c = 0, d = 0;
  if (rocprim::radix_sort_pairs(nullptr, a, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                (size_t)m, 0u, 64u, st) != hipSuccess ||
      rocprim::radix_sort_pairs(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                (size_t)m, 0u, LF_PLACE_BITS, st) != hipSuccess ||
      rocprim::inclusive_scan(nullptr, c, (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)m, rocprim::maximum<uint32_t>(), st) !=
          hipSuccess ||
      rocprim::exclusive_scan(nullptr, d, (const uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)m, rocprim::plus<uint32_t>(), st) !=
          hipSuccess)
    return -1;
  return (int64_t)std::max(std::max(a, b), std::max(c, d));
}

template <bool SB>
static bool fd_launch(const uint4 *rec, uint32_t m, const kv_dev *d_kv, const dint_fold_scratch &s, hipStream_t st, hipEvent_t mid) {
  const dim3 g(fd_grid(m)), tb(FD_TB);
  size_t bytes = s.tmp_bytes;
  hipLaunchKernelGGL(k_fold_keys, g, tb, 0, st, rec, m, d_kv, s.k0, s.i0, s.place_log);
  if (rocprim::radix_sort_pairs(s.tmp, bytes, (const uint64_t *)s.k0, s.k1, (const uint32_t *)s.i0, s.i1, (size_t)m, 0u, 64u, st) != hipSuccess)
    return false;
  hipLaunchKernelGGL(k_fold_place, g, tb, 0, st, (const uint64_t *)s.place_log, (const uint32_t *)s.i1, m, s.k0);
  bytes = s.tmp_bytes;
  if (rocprim::radix_sort_pairs(s.tmp, bytes, (const uint64_t *)s.k0, s.k1, (const uint32_t *)s.i1, s.i0, (size_t)m, 0u, LF_PLACE_BITS, st) !=
      hipSuccess)
    return false;
  const uint64_t *place_s = s.k1;
  const uint32_t *idx_s = s.i0;
  if (mid && hipEventRecord(mid, st) != hipSuccess) return false;
  hipLaunchKernelGGL((k_fold_gather<SB>), g, tb, 0, st, rec, idx_s, m, s.key_s, s.del_s, s.delpos);
  hipLaunchKernelGGL(k_fold_heads, g, tb, 0, st, place_s, (const uint64_t *)s.key_s, m, s.flag);
  bytes = s.tmp_bytes;
  if (rocprim::inclusive_scan(s.tmp, bytes, (const uint32_t *)s.flag, s.rowid, (size_t)m, rocprim::plus<uint32_t>(), st) != hipSuccess) return false;
  bytes = s.tmp_bytes;
  if (rocprim::inclusive_scan(s.tmp, bytes, (const uint32_t *)s.delpos, s.lastdel, (size_t)m, rocprim::maximum<uint32_t>(), st) != hipSuccess)
    return false;
  hipLaunchKernelGGL(k_fold_rows, g, tb, 0, st, (const uint32_t *)s.flag, (const uint32_t *)s.rowid, m, s.row_start, s.words);
  hipLaunchKernelGGL(k_fold_probe, g, tb, 0, st, d_kv, place_s, (const uint64_t *)s.key_s, (const uint32_t *)s.row_start,
                     (const uint32_t *)s.words, s.row_occ, s.row_v0);
  hipLaunchKernelGGL(k_fold_bucket, g, tb, 0, st, place_s, (const uint32_t *)s.row_start, (const uint32_t *)s.words,
                     (const uint32_t *)s.row_occ, s.row_defer, s.counts);
  hipLaunchKernelGGL((k_fold_net<SB>), g, tb, 0, st, m, (const uint32_t *)s.row_start, (const uint32_t *)s.words, (const uint32_t *)s.lastdel,
                     (const uint32_t *)s.row_occ, (const uint32_t *)s.row_v0, (const uint8_t *)s.row_defer, s.row_kind, s.row_ver, s.has);
  bytes = s.tmp_bytes;
  if (rocprim::exclusive_scan(s.tmp, bytes, (const uint32_t *)s.has, s.epos, 0u, (size_t)m, rocprim::plus<uint32_t>(), st) != hipSuccess) return false;
  hipLaunchKernelGGL((k_fold_emit<SB>), g, tb, 0, st, rec, idx_s, place_s, (const uint64_t *)s.key_s, (const uint32_t *)s.row_start,
                     (const uint32_t *)s.words, (const uint32_t *)s.row_kind, (const uint32_t *)s.row_ver, (const uint32_t *)s.has,
                     (const uint32_t *)s.epos, (uint4 *)s.repair);
  hipLaunchKernelGGL((k_fold_count<SB>), g, tb, 0, st, m, idx_s, (const uint32_t *)s.flag, (const uint32_t *)s.rowid, (const uint8_t *)s.del_s,
                     (const uint32_t *)s.row_occ, (const uint8_t *)s.row_defer, s.dflag, s.counts);
  bytes = s.tmp_bytes;
  if (rocprim::exclusive_scan(s.tmp, bytes, (const uint32_t *)s.dflag, s.dpos, 0u, (size_t)m, rocprim::plus<uint32_t>(), st) != hipSuccess) return false;
  hipLaunchKernelGGL(k_fold_defer, dim3(fd_grid((uint64_t)m * 4)), tb, 0, st, rec, m, (const uint32_t *)s.dflag, (const uint32_t *)s.dpos,
                     (uint4 *)s.def_rec);
  hipLaunchKernelGGL(k_fold_totals, dim3(1), dim3(64), 0, st, m, (const uint32_t *)s.dflag, (const uint32_t *)s.dpos, (const uint32_t *)s.has,
                     (const uint32_t *)s.epos, s.words, s.counts);
  return true;
}

bool dint_launch_fold(const void *d_rec, uint32_t m, uint32_t workload, const kv_dev *d_kv, dint_fold_scratch s, hipStream_t st,
                      hipEvent_t mid) {
  if (m == 0 || m > s.cap) return m == 0;
  return workload == DINT_WL_SMALLBANK ? fd_launch<true>((const uint4 *)d_rec, m, d_kv, s, st, mid)
                                       : fd_launch<false>((const uint4 *)d_rec, m, d_kv, s, st, mid);
}

void dint_launch_fold_rotate(const kv_dev *d_kv, hipStream_t st) {
  hipLaunchKernelGGL(k_fold_rotate, dim3(1), dim3(KV_NLISTS), 0, st, d_kv);
}

void dint_launch_fold_harvest(const unsigned long long *repair_words, dint_fold_scratch s, hipStream_t st) {
  hipLaunchKernelGGL(k_fold_harvest, dim3(1), dim3(64), 0, st, repair_words, s.counts);
}

// ---- the host form (include/dint_driver.h): the same log_fold.h functions over dumped rows and plain arrays ------------------
extern "C" int64_t dint_log_fold_host(uint32_t workload, uint32_t n_tables, const uint64_t *hash_size, const uint64_t *row_off,
                                      const uint64_t *keys, const uint32_t *vers, const void *records, uint64_t n, uint8_t *deferred_out,
                                      void *repair_out, uint64_t cap, dint_fold_stats *out) {
  if ((workload != DINT_WL_TATP && workload != DINT_WL_SMALLBANK) || n_tables == 0 || n_tables > 5 || !hash_size || !row_off ||
      (row_off[n_tables] && (!keys || !vers)) || (n && (!records || !deferred_out)) || (cap && !repair_out) || n > 0xFFFFFFFFull)
    return DINT_EINVAL;
  for (uint32_t t = 0; t < n_tables; t++)
    if (hash_size[t] == 0 || hash_size[t] > 0xFFFFFFFFull || row_off[t] > row_off[t + 1]) return DINT_EINVAL;
  const bool sb = workload == DINT_WL_SMALLBANK;
  const LrRecord *rec = (const LrRecord *)records;
  if (out) memset(out, 0, sizeof *out);
  if (n == 0) return 0;
  try {
    struct seen { uint32_t occ, v0; };
    std::vector<std::unordered_map<uint64_t, seen>> rows(n_tables);  // per key: slots that hold it, the version of the first in dump order
    for (uint32_t t = 0; t < n_tables; t++)
      for (uint64_t j = row_off[t]; j < row_off[t + 1]; j++) {
        auto it = rows[t].find(keys[j]);
        if (it == rows[t].end()) rows[t].emplace(keys[j], seen{1u, vers[j]});
        else it->second.occ++;
      }
    std::vector<dint_mod> mod(n_tables);
    for (uint32_t t = 0; t < n_tables; t++) mod[t] = dint_make_mod(hash_size[t]);
    std::vector<uint64_t> place(n);
    std::vector<uint32_t> idx(n);
    for (uint64_t i = 0; i < n; i++)
      place[i] = rec[i].table < n_tables ? lf_place(rec[i].table, rr_local(rec[i].key, rec[i].table, mod.data(), 0, 1))  // (the host form: unsharded)
                                         : lf_place(LF_BAD_TABLE, 0);
    std::iota(idx.begin(), idx.end(), 0u);
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) {
      return place[x] != place[y] ? place[x] < place[y] : rec[x].key < rec[y].key;
    });
    uint64_t c[DINT_FOLD_COUNTS] = {0};
    uint64_t emitted = 0;
    for (uint64_t b0 = 0; b0 < n;) {  // one bucket of the chunk
      uint64_t b1 = b0;
      while (b1 < n && place[idx[b1]] == place[idx[b0]]) b1++;
      const uint32_t table = lf_place_table(place[idx[b0]]);
      struct row { uint64_t s, e; uint32_t occ, v0; };
      std::vector<row> rs;
      bool deferred = false;
      for (uint64_t s = b0; s < b1;) {
        uint64_t e = s;
        while (e < b1 && rec[idx[e]].key == rec[idx[s]].key) e++;
        seen f = {0u, 0u};
        if (table >= n_tables) {
          f.occ = 2;
        } else {
          auto it = rows[table].find(rec[idx[s]].key);
          if (it != rows[table].end()) f = it->second;
        }
        deferred |= lf_defers(f.occ);
        rs.push_back(row{s, e, f.occ, f.v0});
        s = e;
      }
      c[8] += rs.size();
      if (deferred) c[7]++;
      for (const row &r : rs) {
        uint32_t scan = 0;  // the max-scan's value at the row's last position, positions counted from the row's first
        for (uint64_t p = r.s; p < r.e; p++) {
          const LrRecord &x = rec[idx[p]];
          const uint8_t del = sb ? (uint8_t)0 : (uint8_t)(x.is_del != 0);
          const bool first = p == r.s;
          const uint8_t prev = first ? (uint8_t)0 : (uint8_t)(!sb && rec[idx[p - 1]].is_del != 0);
          c[(deferred ? 3 : 0) + lf_kind(sb, del, first, r.occ, prev)]++;
          deferred_out[idx[p]] = deferred;
          if (del) scan = (uint32_t)(p - r.s) + 1u;
        }
        if (deferred) {
          c[6] += r.e - r.s;
          continue;
        }
        const lf_net net = lf_fold(sb, r.occ, r.v0, (uint32_t)(r.e - r.s), sb ? 0u : lf_last_delete(scan, 0u));
        if (net.kind == LF_NONE) continue;
        if (emitted < cap) {
          uint32_t last[16], w[16];
          memcpy(last, &rec[idx[r.e - 1]], 64);
          lf_record(w, sb, net, rec[idx[r.s]].key, table, last);
          memcpy((uint8_t *)repair_out + emitted * 64, w, 64);
        }
        emitted++;
      }
      b0 = b1;
    }
    if (out) {
      out->commits = c[0] + c[3]; out->inserts = c[1] + c[4]; out->deletes = c[2] + c[5];
      out->applied = n;
      out->chunks = 1;
      out->rows = c[8];
      out->deferred_records = c[6];
      out->folded_records = n - c[6];
      out->deferred_buckets = c[7];
      out->repair_records = emitted;
    }
    return (int64_t)std::min(emitted, cap);
  } catch (const std::bad_alloc &) {
    return DINT_ENOMEM;
  }
}
