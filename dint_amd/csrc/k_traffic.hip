// k_traffic.hip -- a batch's hot keys, reply codes and shared lock slots, read where the batch lies (include/dint_abi.h
// struct dint_traffic_report, driven by engine.hip; the rule lives in traffic_report.h, which the host form at the end of this file shares).
//
//   k_tr_decode        a tile of TRK_TILE messages staged through LDS: the byte range of the tile is cut at the 16-byte boundaries of
//                      its ADDRESS -- head and tail bytes go byte by byte, the body as 16-byte vectors, and the LDS copy sits at the
//                      same offset modulo 16, so that both sides of every vector are aligned whatever the array's address.  Nothing
//                      outside [array, array + n * msg) is read.  Per request it emits key, meta word (class, table, flags), its index
//                      and the table byte the second sort goes by.  The replies of the tile are staged the same way behind the
//                      requests; only their type byte is used.  The two type histograms and the ten scalar counts stay in LDS while
//                      the workgroup strides over its tiles and leave as ONE partial of TRK_PART words;
//   k_tr_decode_sum    one workgroup adds the partials up, thread w word w (k_stats.hip's shape).  No global atomic, no order.
//   (host)             synchronisation 1: the keyed count K.
//   rocprim            stable radix sort of (key, index) by key, then -- workloads with a table byte -- of (table, index) by table:
//                      the keyed requests are the first K, in (table, key, index) order; requests that are not keyed carry table 7.
//                      No sentinel KEY anywhere: 0 and 2^64 - 1 sort like any other.
//   k_tr_heads         run heads of (table, key); rocprim inclusive scan = the 1-based number of a request's distinct key
//   k_tr_key_reduce    a tile of 256 sorted requests adds its counters per run in LDS and then once per (tile, run) to the run's
//                      list entry: n / 256 + distinct keys atomic adds at most, all integer -- the result does not depend on order.
//                      The run's head writes key, table and first_index (both sorts are stable: the head has the lowest index).
//   (host)             synchronisation 2: the distinct keys D.
//   k_tr_key_stats     per distinct key: the per-key histogram and maximum, its unit and lock-slot words, the two top-list sort keys
//   groups             twice (units; lock slots): rocprim sort of (group word, key number), heads, scan, the same tile reduce over
//                      {keys, requests, rejects}, and k_tr_group_stats: distinct, shared_*, the per-unit histogram and the maximum
//                      as one 64-bit atomicMax of requests << 32 | ~position (the list is ascending: the lowest unit wins a tie)
//   top lists          the entries are in (table, key) order already: a stable sort by the complemented count gives the contract's
//                      order; the first K entries are copied.  Twice.
//   (host)             synchronisation 3: the result words and the lists.
// Every kernel's index is bounded by a count its caller passed or that it reads from the words of the stage before; no workgroup
// waits for another.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "../../include/dint_abi.h"
#include "../../include/dint_driver.h"
#include "dint_kv.h"
#include "dint_traffic.h"
#include "traffic_report.h"

#define TRK_TB 256u
#define TRK_TILE 512u                         // messages per tile of the decode stage
#define TRK_GRID 1024u                        // its workgroups at most; they stride over the tiles
#define TRK_MAX_MSG 55u
#define TRK_STAGE_BYTES ((TRK_TILE * TRK_MAX_MSG + 15u + 15u) & ~15u)  // a tile at any offset modulo 16
#define TRK_HIST (2u * TR_MAX_TABLES * TR_TYPE_BINS)
#define TRK_SCALARS 10u                       // keyed, bad_table, log, reads, locks, unlocks, writes, others, rejects, misses
#define TRK_PART (TRK_HIST + TRK_SCALARS)
#define TRK_SUM_TB 384u
#define TRK_RUN_FIELDS 9u                     // requests, reads, locks, unlocks, writes, rejects, misses, slot requests, slot rejects
// control words behind the report's
enum : uint32_t { TRX_MAXPACK = TR_WORDS, TRX_NREJ, TRX_WORDS_END = TR_WORDS + 8 };

static_assert(TRK_PART <= TRK_SUM_TB && TRK_STAGE_BYTES + TRK_PART * 4u + 64u <= 65536u, "the decode stage stays within 64 KB of LDS");
static_assert(TR_W_KEYED + TRK_SCALARS - 1 == TR_W_MISSES, "the ten scalars are consecutive report words");

// `bytes` bytes from src to lds + (src & 15): 16-byte vectors between the 16-byte boundaries of the address, single bytes outside
__device__ static inline uint32_t trk_stage(uint8_t *lds, const uint8_t *__restrict__ src, uint32_t bytes) {
  const uint32_t tid = threadIdx.x;
  const uint32_t o = (uint32_t)((uintptr_t)src & 15u);
  const uint32_t head = o ? min(16u - o, bytes) : 0u;
  const uint32_t body = (bytes - head) & ~15u;
  for (uint32_t k = tid; k < head; k += TRK_TB) lds[o + k] = src[k];
  const uint4 *gs = (const uint4 *)(src + head);
  uint4 *ls = (uint4 *)(lds + o + head);
  for (uint32_t v = tid; v < body / 16u; v += TRK_TB) ls[v] = gs[v];
  for (uint32_t k = head + body + tid; k < bytes; k += TRK_TB) lds[o + k] = src[k];
  return o;
}

// lanes of the wave for which `c` holds, added to *w by lane 0
__device__ static inline void trk_count(uint32_t *w, bool c) {
  const uint64_t m = __ballot(c);
  if ((threadIdx.x & 63u) == 0 && m) atomicAdd(w, (uint32_t)__popcll(m));
}

__global__ void __launch_bounds__(TRK_TB)
k_tr_decode(const uint8_t *__restrict__ req, const uint8_t *__restrict__ rep, uint32_t n, tr_geom g, uint64_t *__restrict__ key,
            uint32_t *__restrict__ meta, uint32_t *__restrict__ idx, uint8_t *__restrict__ tab, uint32_t *__restrict__ part) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[TRK_STAGE_BYTES];
  __shared__ uint32_t acc[TRK_PART];
  const uint32_t tid = threadIdx.x;
  const tr_format f = tr_format_of(g.workload);
  for (uint32_t w = tid; w < TRK_PART; w += TRK_TB) acc[w] = 0;
  const uint32_t tiles = (n + TRK_TILE - 1) / TRK_TILE;
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // (uniform in the workgroup)
    const uint32_t first = tile * TRK_TILE, tile_n = min(TRK_TILE, n - first);
    __syncthreads();  // the previous tile's bytes have been read; acc is zero
    uint32_t o = trk_stage(stage, req + (size_t)first * f.msg, tile_n * f.msg);
    __syncthreads();
    uint64_t k[TRK_TILE / TRK_TB];
    uint32_t m[TRK_TILE / TRK_TB], t[TRK_TILE / TRK_TB], y[TRK_TILE / TRK_TB];
#pragma unroll
    for (uint32_t j = 0; j < TRK_TILE / TRK_TB; j++) {
      const uint32_t r = tid + j * TRK_TB;
      m[j] = 0; t[j] = TR_NOT_KEYED; y[j] = 0; k[j] = 0;
      if (r < tile_n) {
        uint32_t yr;
        const uint8_t *p = stage + o + r * f.msg;
        m[j] = tr_decode(g, f, p, p, false, &k[j], &t[j], &y[j], &yr);
      }
    }
    if (rep) {
      __syncthreads();
      o = trk_stage(stage, rep + (size_t)first * f.msg, tile_n * f.msg);
      __syncthreads();
    }
#pragma unroll
    for (uint32_t j = 0; j < TRK_TILE / TRK_TB; j++) {
      const uint32_t r = tid + j * TRK_TB;
      const bool live = r < tile_n;
      const bool in_table = live && t[j] < g.n_tables;
      const uint32_t mt = m[j] >> TR_M_TABLE_SHIFT & 7u, c = m[j] & TR_M_CLASS;
      const bool keyed = live && mt != TR_NOT_KEYED;
      if (rep && in_table) {
        const uint32_t yr = stage[o + r * f.msg + f.type];
        atomicAdd(&acc[TRK_HIST / 2 + t[j] * TR_TYPE_BINS + tr_type_bin(yr)], 1u);
        if (keyed) m[j] |= tr_reply_flags(g.workload, yr);
      }
      if (in_table) atomicAdd(&acc[t[j] * TR_TYPE_BINS + tr_type_bin(y[j])], 1u);
      uint32_t *s = acc + TRK_HIST;
      trk_count(s + 0, keyed);
      trk_count(s + 1, live && !in_table);
      trk_count(s + 2, in_table && c == TR_LOG);
      trk_count(s + 3, keyed && c == TR_READ);
      trk_count(s + 4, keyed && c == TR_LOCK);
      trk_count(s + 5, keyed && c == TR_UNLOCK);
      trk_count(s + 6, keyed && c == TR_WRITE);
      trk_count(s + 7, keyed && c == TR_OTHER);
      trk_count(s + 8, keyed && (m[j] & TR_M_REJECT));
      trk_count(s + 9, keyed && (m[j] & TR_M_MISS));
      if (live) {
        const uint32_t i = first + r;
        key[i] = k[j];
        meta[i] = m[j];
        idx[i] = i;
        tab[i] = (uint8_t)mt;
      }
    }
  }
  __syncthreads();
  for (uint32_t w = tid; w < TRK_PART; w += TRK_TB) part[(size_t)TRK_PART * blockIdx.x + w] = acc[w];
}

__global__ void __launch_bounds__(TRK_SUM_TB) k_tr_decode_sum(const uint32_t *__restrict__ part, uint32_t parts, unsigned long long *__restrict__ words) {
  const uint32_t w = threadIdx.x;
  if (w >= TRK_PART) return;
  unsigned long long v = 0;
  for (uint32_t p = 0; p < parts; p++) v += part[(size_t)TRK_PART * p + w];
  const uint32_t at = w < TRK_HIST / 2 ? TR_W_REQ_TYPES + w : w < TRK_HIST ? TR_W_REP_TYPES + (w - TRK_HIST / 2) : TR_W_KEYED + (w - TRK_HIST);
  words[at] = v;
}

// tab1[j] = tab[idx1[j]]: the second sort's keys in the first sort's order
__global__ void __launch_bounds__(TRK_TB) k_tr_gather_tab(const uint8_t *__restrict__ tab, const uint32_t *__restrict__ idx1, uint32_t n, uint8_t *__restrict__ tab1) {
  const uint32_t j = blockIdx.x * TRK_TB + threadIdx.x;
  if (j < n) tab1[j] = tab[idx1[j]];
}

// head[j] = sorted request j opens a run of (table, key); j < K
__global__ void __launch_bounds__(TRK_TB) k_tr_heads(const uint64_t *__restrict__ key, const uint32_t *__restrict__ meta, const uint32_t *__restrict__ perm,
                                                     uint32_t K, uint32_t *__restrict__ head) {
  const uint32_t j = blockIdx.x * TRK_TB + threadIdx.x;
  if (j >= K) return;
  const uint32_t i = perm[j];
  uint32_t h = 1;
  if (j) {
    const uint32_t p = perm[j - 1];
    h = key[i] != key[p] || ((meta[i] ^ meta[p]) >> TR_M_TABLE_SHIFT & 7u) != 0;
  }
  head[j] = h;
}

// the counters of sorted requests [256 b, 256 b + 256) added to their runs' entries
__global__ void __launch_bounds__(TRK_TB)
k_tr_key_reduce(const uint64_t *__restrict__ key, const uint32_t *__restrict__ meta, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ head,
                const uint32_t *__restrict__ seg, uint32_t K, dint_traffic_key *__restrict__ ent, uint32_t *__restrict__ sreq, uint32_t *__restrict__ srej) {
  __shared__ uint32_t cnt[TRK_TB][TRK_RUN_FIELDS];
  const uint32_t tid = threadIdx.x, first = blockIdx.x * TRK_TB, j = first + tid;
  for (uint32_t x = tid; x < TRK_TB * TRK_RUN_FIELDS; x += TRK_TB) (&cnt[0][0])[x] = 0;
  __syncthreads();
  const uint32_t base = seg[first] - 1u;  // (first < K: the grid is ceil(K / 256); seg >= 1)
  if (j < K) {
    const uint32_t i = perm[j], m = meta[i], run = seg[j] - 1u, l = run - base, c = m & TR_M_CLASS;  // l <= tid
    atomicAdd(&cnt[l][0], 1u);
    if (c <= TR_WRITE) atomicAdd(&cnt[l][1 + c], 1u);
    if (m & TR_M_REJECT) atomicAdd(&cnt[l][5], 1u);
    if (m & TR_M_MISS) atomicAdd(&cnt[l][6], 1u);
    if (m & TR_M_SLOT) {
      atomicAdd(&cnt[l][7], 1u);
      if (m & TR_M_REJECT) atomicAdd(&cnt[l][8], 1u);
    }
    if (head[j]) {
      ent[run].key = key[i];
      ent[run].table = m >> TR_M_TABLE_SHIFT & 7u;
      ent[run].first_index = i;
    }
  }
  __syncthreads();
  for (uint32_t x = tid; x < TRK_TB * TRK_RUN_FIELDS; x += TRK_TB) {
    const uint32_t l = x / TRK_RUN_FIELDS, fld = x % TRK_RUN_FIELDS, v = cnt[l][fld];
    if (v) {  // (only runs that have a request in the tile: base + l < the distinct keys)
      uint32_t *dst = fld < 7 ? &ent[base + l].requests + fld : fld == 7 ? &sreq[base + l] : &srej[base + l];
      atomicAdd(dst, v);
    }
  }
}
static_assert(offsetof(dint_traffic_key, requests) == 12 && offsetof(dint_traffic_key, misses) == 36 && offsetof(dint_traffic_key, first_index) == 40,
              "requests, reads, locks, unlocks, writes, rejects, misses are seven consecutive words");

__device__ static inline unsigned long long trk_wave_sum(unsigned long long v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, d, 64), hi = __shfl_xor((uint32_t)(v >> 32), d, 64);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}
__device__ static inline void trk_wave_add(unsigned long long *w, unsigned long long v) {
  v = trk_wave_sum(v);
  if ((threadIdx.x & 63u) == 0 && v) atomicAdd(w, v);
}

// per distinct key d < D: the per-key histogram and maximum, the unit and lock-slot words, the two sort keys of the top lists
__global__ void __launch_bounds__(TRK_TB)
k_tr_key_stats(const dint_traffic_key *__restrict__ ent, const uint32_t *__restrict__ sreq, uint32_t D, tr_geom g, uint32_t slots,
               uint64_t *__restrict__ ukey, uint64_t *__restrict__ lkey, uint32_t *__restrict__ rk, uint32_t *__restrict__ jk, unsigned long long *words) {
  __shared__ uint32_t hist[TR_HIST_BINS];
  const uint32_t tid = threadIdx.x, d = blockIdx.x * TRK_TB + tid;
  if (tid < TR_HIST_BINS) hist[tid] = 0;
  __syncthreads();
  uint32_t req = 0, rej = 0;
  if (d < D) {
    const dint_traffic_key e = ent[d];
    req = e.requests;
    rej = e.rejects;
    atomicAdd(&hist[tr_count_bin(req)], 1u);
    ukey[d] = tr_unit(g, e.table, e.key);
    if (slots) lkey[d] = sreq[d] ? tr_slot(g, e.table, e.key) : TR_NO_GROUP;
    rk[d] = ~req;
    jk[d] = ~rej;
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) req = max(req, (uint32_t)__shfl_xor(req, s, 64));
  if ((tid & 63u) == 0 && req) atomicMax(&words[TR_W_MAX_KEY], (unsigned long long)req);
  trk_wave_add(&words[TRX_NREJ], rej ? 1ull : 0ull);
  __syncthreads();
  if (tid < TR_HIST_BINS && hist[tid]) atomicAdd(&words[TR_W_KEY_HIST + tid], (unsigned long long)hist[tid]);
}

// head[j] = sorted group word j opens a group (TR_NO_GROUP words sort last and open none)
__global__ void __launch_bounds__(TRK_TB) k_tr_group_heads(const uint64_t *__restrict__ gkey, uint32_t D, uint32_t *__restrict__ head) {
  const uint32_t j = blockIdx.x * TRK_TB + threadIdx.x;
  if (j >= D) return;
  const uint64_t k = gkey[j];
  head[j] = k != TR_NO_GROUP && (j == 0 || gkey[j - 1] != k);
}

// {keys, requests, rejects} of sorted keys [256 b, 256 b + 256) added to their groups; slot: the lock-slot requests and rejects
__global__ void __launch_bounds__(TRK_TB)
k_tr_group_reduce(const uint64_t *__restrict__ gkey, const uint32_t *__restrict__ gidx, const uint32_t *__restrict__ head, const uint32_t *__restrict__ seg,
                  uint32_t D, const dint_traffic_key *__restrict__ ent, const uint32_t *__restrict__ sreq, const uint32_t *__restrict__ srej, uint32_t slot,
                  uint32_t *__restrict__ gcnt, uint64_t *__restrict__ gk_out) {
  __shared__ uint32_t cnt[TRK_TB][3];
  const uint32_t tid = threadIdx.x, first = blockIdx.x * TRK_TB, j = first + tid;
  if (gkey[first] == TR_NO_GROUP) return;  // (uniform: sorted, so the whole tile is without a group)
  for (uint32_t x = tid; x < TRK_TB * 3u; x += TRK_TB) (&cnt[0][0])[x] = 0;
  __syncthreads();
  const uint32_t base = seg[first] - 1u;
  if (j < D && gkey[j] != TR_NO_GROUP) {
    const uint32_t d = gidx[j], grp = seg[j] - 1u, l = grp - base;
    atomicAdd(&cnt[l][0], 1u);
    atomicAdd(&cnt[l][1], slot ? sreq[d] : ent[d].requests);
    const uint32_t rj = slot ? srej[d] : ent[d].rejects;
    if (rj) atomicAdd(&cnt[l][2], rj);
    if (head[j]) gk_out[grp] = gkey[j];
  }
  __syncthreads();
  for (uint32_t x = tid; x < TRK_TB * 3u; x += TRK_TB) {
    const uint32_t v = (&cnt[0][0])[x];
    if (v) atomicAdd(&gcnt[(size_t)(base + x / 3u) * 3u + x % 3u], v);
  }
}

// per group u < G = seg[D - 1]: distinct, shared_*; units also the histogram and the maximum
__global__ void __launch_bounds__(TRK_TB)
k_tr_group_stats(const uint32_t *__restrict__ gcnt, const uint32_t *__restrict__ seg, uint32_t D, uint32_t slot, unsigned long long *words) {
  __shared__ uint32_t hist[TR_HIST_BINS];
  const uint32_t tid = threadIdx.x, u = blockIdx.x * TRK_TB + tid, G = seg[D - 1];
  if (tid < TR_HIST_BINS) hist[tid] = 0;
  __syncthreads();
  unsigned long long one = 0, sh = 0, shreq = 0, shrej = 0, pack = 0;
  if (u < G) {
    const uint32_t keys = gcnt[(size_t)u * 3], req = gcnt[(size_t)u * 3 + 1], rej = gcnt[(size_t)u * 3 + 2];
    one = 1;
    if (keys >= 2) { sh = 1; shreq = req; shrej = rej; }
    if (!slot) {
      atomicAdd(&hist[tr_count_bin(req)], 1u);
      pack = (unsigned long long)req << 32 | (0xFFFFFFFFu - u);
    }
  }
  trk_wave_add(&words[slot ? TR_W_DSLOTS : TR_W_DUNITS], one);
  trk_wave_add(&words[slot ? TR_W_SH_SLOTS : TR_W_SH_UNITS], sh);
  trk_wave_add(&words[slot ? TR_W_SH_SLOT_REQ : TR_W_SH_UNIT_REQ], shreq);
  trk_wave_add(&words[slot ? TR_W_SH_SLOT_REJ : TR_W_SH_UNIT_REJ], shrej);
  if (!slot) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
      const uint32_t lo = __shfl_xor((uint32_t)pack, s, 64), hi = __shfl_xor((uint32_t)(pack >> 32), s, 64);
      const unsigned long long o = ((unsigned long long)hi << 32) | lo;
      pack = pack > o ? pack : o;
    }
    if ((tid & 63u) == 0 && pack) atomicMax(&words[TRX_MAXPACK], pack);
    __syncthreads();
    if (tid < TR_HIST_BINS && hist[tid]) atomicAdd(&words[TR_W_UNIT_HIST + tid], (unsigned long long)hist[tid]);
  }
}
__global__ void k_tr_max_unit(const uint64_t *__restrict__ gk_out, unsigned long long *words) {
  const unsigned long long pack = words[TRX_MAXPACK];
  if (threadIdx.x || blockIdx.x || !pack) return;
  const uint64_t gk = gk_out[0xFFFFFFFFu - (uint32_t)pack];
  words[TR_W_MAX_UNIT_REQ] = pack >> 32;
  words[TR_W_MAX_UNIT] = gk & ((1ull << TR_GROUP_TABLE_SHIFT) - 1);
  words[TR_W_MAX_UNIT_TABLE] = gk >> TR_GROUP_TABLE_SHIFT;
}

// top[r] = ent[order[r]] for r < min(top_k, D, *limit)  (limit: the keys with a reject, or nullptr)
__global__ void __launch_bounds__(TRK_TB)
k_tr_emit(const dint_traffic_key *__restrict__ ent, const uint32_t *__restrict__ order, uint32_t D, uint32_t top_k, const unsigned long long *limit,
          dint_traffic_key *__restrict__ top) {
  const uint32_t r = blockIdx.x * TRK_TB + threadIdx.x;
  unsigned long long m = min(top_k, D);
  if (limit && *limit < m) m = *limit;
  if (r < m) top[r] = ent[order[r]];
}

// ------------------------------------------------------------------------------------------------------ host side
#define TR_HIP(x)                                                                     \
  do {                                                                                \
    hipError_t e_ = (x);                                                              \
    if (e_ != hipSuccess) {                                                           \
      char m_[200];                                                                   \
      snprintf(m_, sizeof m_, "traffic report: %s: %s", #x, hipGetErrorString(e_));   \
      dint_set_last_error(m_);                                                        \
      return DINT_EHIP;                                                               \
    }                                                                                 \
  } while (0)

bool dint_traffic_geom(uint32_t workload, uint64_t n_slots, uint64_t n_rows, uint32_t flags, tr_geom *g) {
  (void)flags;  // (no dint_config flag changes a bucket count; dint_kv_hash_sizes is the one place that would follow one)
  memset(g, 0, sizeof *g);
  g->workload = workload;
  if (!tr_workload_ok(workload)) return false;
  uint64_t hs[DINT_KV_MAX_TABLES] = {0, 0, 0, 0, 0};
  if (workload == DINT_WL_FASST || workload == DINT_WL_2PL) {
    g->n_tables = 1;
    hs[0] = n_slots ? n_slots : 36000000ull;  // lock_fasst/udp/utils.h:12, as dint_engine_create
  } else {
    uint32_t val_size;
    g->n_tables = dint_kv_hash_sizes(workload, n_rows, hs, &val_size);
  }
  for (uint32_t t = 0; t < TR_MAX_TABLES; t++) {
    g->unit[t] = dint_make_mod(t < g->n_tables ? hs[t] : 1);
    g->slot[t] = dint_make_mod(t < g->n_tables ? 4 * hs[t] : 1);
  }
  return true;
}

void dint_traffic_free(dint_traffic_scratch &s) {
  if (s.arena) (void)hipFree(s.arena);
  if (s.words) (void)hipFree(s.words);
  if (s.part) (void)hipFree(s.part);
  if (s.top) (void)hipFree(s.top);
  s = dint_traffic_scratch{};
}

namespace {
struct tr_arena {  // the arrays of one call, carved from the arena in 256-byte steps
  size_t at = 0;
  size_t take(size_t bytes) {
    const size_t o = at;
    at += (bytes + 255) & ~(size_t)255;
    return o;
  }
};
struct tr_arrays {
  size_t key, meta, idx0, tab, key_s, idx1, tab1, tab2, idx2, head, seg, ent, sreq, srej, ukey, lkey, gcnt, gk_out, rk, jk, tmp, total;
  size_t tmp_bytes;
};
int tr_tmp_bytes(uint64_t n, hipStream_t st, size_t *out) {
  size_t a = 0, b = 0, c = 0, d = 0;
  TR_HIP(rocprim::radix_sort_pairs(nullptr, a, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n, 0u, 64u, st));
  TR_HIP(rocprim::radix_sort_pairs(nullptr, b, (const uint8_t *)nullptr, (uint8_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n, 0u, 3u, st));
  TR_HIP(rocprim::radix_sort_pairs(nullptr, c, (const uint32_t *)nullptr, (uint32_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n, 0u, 25u, st));
  TR_HIP(rocprim::inclusive_scan(nullptr, d, (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n, rocprim::plus<uint32_t>(), st));
  *out = std::max(std::max(a, b), std::max(c, d)) + 4096;
  return 0;
}
int tr_layout(uint64_t n, hipStream_t st, tr_arrays *l) {
  if (int rc = tr_tmp_bytes(n, st, &l->tmp_bytes)) return rc;
  tr_arena a;
  l->key = a.take(8 * n); l->meta = a.take(4 * n); l->idx0 = a.take(4 * n); l->tab = a.take(n);
  l->key_s = a.take(8 * n); l->idx1 = a.take(4 * n); l->tab1 = a.take(n); l->tab2 = a.take(n); l->idx2 = a.take(4 * n);
  l->head = a.take(4 * n); l->seg = a.take(4 * n);
  l->ent = a.take(sizeof(dint_traffic_key) * n); l->sreq = a.take(4 * n); l->srej = a.take(4 * n);
  l->ukey = a.take(8 * n); l->lkey = a.take(8 * n); l->gcnt = a.take(12 * n); l->gk_out = a.take(8 * n);
  l->rk = a.take(4 * n); l->jk = a.take(4 * n);
  l->tmp = a.take(l->tmp_bytes);
  l->total = a.at;
  return 0;
}
// rocprim calls that first ask what THIS size needs: the temporary storage was sized for n, the largest of a call
template <class K>
int tr_sort(void *tmp, size_t cap, const K *kin, K *kout, const uint32_t *vin, uint32_t *vout, size_t n, unsigned b0, unsigned b1, hipStream_t st) {
  size_t need = 0;
  TR_HIP(rocprim::radix_sort_pairs(nullptr, need, kin, kout, vin, vout, n, b0, b1, st));
  if (need > cap) {
    dint_set_last_error("traffic report: a sort needs more temporary storage than the call reserved (an internal error)");
    return DINT_EHIP;
  }
  TR_HIP(rocprim::radix_sort_pairs(tmp, need, kin, kout, vin, vout, n, b0, b1, st));
  return 0;
}
int tr_scan(void *tmp, size_t cap, const uint32_t *in, uint32_t *out, size_t n, hipStream_t st) {
  size_t need = 0;
  TR_HIP(rocprim::inclusive_scan(nullptr, need, in, out, n, rocprim::plus<uint32_t>(), st));
  if (need > cap) {
    dint_set_last_error("traffic report: a scan needs more temporary storage than the call reserved (an internal error)");
    return DINT_EHIP;
  }
  TR_HIP(rocprim::inclusive_scan(tmp, need, in, out, n, rocprim::plus<uint32_t>(), st));
  return 0;
}
inline uint32_t tr_blocks(uint64_t n) { return (uint32_t)((n + TRK_TB - 1) / TRK_TB); }
}  // namespace

int dint_traffic_run(const tr_geom &g, dint_traffic_scratch &s, const void *d_req, const void *d_rep, uint64_t n, uint32_t top_k, hipStream_t st,
                     struct dint_traffic_report *out, dint_traffic_key *by_requests, dint_traffic_key *by_rejects) {
  std::vector<unsigned long long> h(TRX_WORDS_END, 0);
  const size_t fixed = (size_t)TRX_WORDS_END * 8 + (size_t)TRK_GRID * TRK_PART * 4 + 2 * (size_t)DINT_TRAFFIC_MAX_TOP * sizeof(dint_traffic_key);
  uint64_t temp = 0, D = 0, nrej = 0;
  if (n) {
    if (!s.words) {
      if (hipMalloc((void **)&s.words, (size_t)TRX_WORDS_END * 8) != hipSuccess || hipMalloc((void **)&s.part, (size_t)TRK_GRID * TRK_PART * 4) != hipSuccess ||
          hipMalloc((void **)&s.top, 2 * (size_t)DINT_TRAFFIC_MAX_TOP * sizeof(dint_traffic_key)) != hipSuccess) {
        dint_traffic_free(s);
        dint_set_last_error("traffic report: out of device memory");
        return DINT_ENOMEM;
      }
    }
    tr_arrays l;
    if (int rc = tr_layout(n, st, &l)) return rc;
    if (l.total > s.arena_bytes) {  // (a caller that hands in a scratch it used before: grown to what this call needs)
      if (s.arena) {
        TR_HIP(hipStreamSynchronize(st));
        (void)hipFree(s.arena);
      }
      s.arena = nullptr;
      s.arena_bytes = 0;
      if (hipMalloc(&s.arena, l.total) != hipSuccess) {
        char m[160];
        snprintf(m, sizeof m, "traffic report: %zu bytes of temporary device memory for %llu requests", l.total, (unsigned long long)n);
        dint_set_last_error(m);
        return DINT_ENOMEM;
      }
      s.arena_bytes = l.total;
    }
    temp = s.arena_bytes + fixed;
    uint8_t *A = (uint8_t *)s.arena;
    uint64_t *key = (uint64_t *)(A + l.key), *key_s = (uint64_t *)(A + l.key_s), *ukey = (uint64_t *)(A + l.ukey), *lkey = (uint64_t *)(A + l.lkey),
             *gk_out = (uint64_t *)(A + l.gk_out);
    uint32_t *meta = (uint32_t *)(A + l.meta), *idx0 = (uint32_t *)(A + l.idx0), *idx1 = (uint32_t *)(A + l.idx1), *idx2 = (uint32_t *)(A + l.idx2),
             *head = (uint32_t *)(A + l.head), *seg = (uint32_t *)(A + l.seg), *sreq = (uint32_t *)(A + l.sreq), *srej = (uint32_t *)(A + l.srej),
             *gcnt = (uint32_t *)(A + l.gcnt), *rk = (uint32_t *)(A + l.rk), *jk = (uint32_t *)(A + l.jk);
    uint8_t *tab = A + l.tab, *tab1 = A + l.tab1, *tab2 = A + l.tab2;
    dint_traffic_key *ent = (dint_traffic_key *)(A + l.ent);
    void *tmp = A + l.tmp;

    // ---- decode, and the counts that need no key
    TR_HIP(hipMemsetAsync(s.words, 0, (size_t)TRX_WORDS_END * 8, st));
    const uint32_t tiles = (uint32_t)((n + TRK_TILE - 1) / TRK_TILE), grid = std::min(tiles, TRK_GRID);
    hipLaunchKernelGGL(k_tr_decode, dim3(grid), dim3(TRK_TB), 0, st, (const uint8_t *)d_req, (const uint8_t *)d_rep, (uint32_t)n, g, key, meta, idx0, tab, s.part);
    hipLaunchKernelGGL(k_tr_decode_sum, dim3(1), dim3(TRK_SUM_TB), 0, st, (const uint32_t *)s.part, grid, s.words);
    TR_HIP(hipGetLastError());
    TR_HIP(hipMemcpyAsync(h.data(), s.words, (size_t)TR_WORDS * 8, hipMemcpyDeviceToHost, st));
    TR_HIP(hipStreamSynchronize(st));  // (1) the keyed requests
    const uint64_t K = h[TR_W_KEYED];
    if (K > n) {
      dint_set_last_error("traffic report: more keyed requests than requests (an internal error)");
      return DINT_EHIP;
    }
    if (K) {
      // ---- the keyed requests in (table, key, index) order
      if (int rc = tr_sort(tmp, l.tmp_bytes, (const uint64_t *)key, key_s, (const uint32_t *)idx0, idx1, (size_t)n, 0u, 64u, st)) return rc;
      const uint32_t *perm = idx1;
      if (g.n_tables > 1) {
        hipLaunchKernelGGL(k_tr_gather_tab, dim3(tr_blocks(n)), dim3(TRK_TB), 0, st, (const uint8_t *)tab, (const uint32_t *)idx1, (uint32_t)n, tab1);
        if (int rc = tr_sort(tmp, l.tmp_bytes, (const uint8_t *)tab1, tab2, (const uint32_t *)idx1, idx2, (size_t)n, 0u, 3u, st)) return rc;
        perm = idx2;
      }
      hipLaunchKernelGGL(k_tr_heads, dim3(tr_blocks(K)), dim3(TRK_TB), 0, st, (const uint64_t *)key, (const uint32_t *)meta, perm, (uint32_t)K, head);
      if (int rc = tr_scan(tmp, l.tmp_bytes, (const uint32_t *)head, seg, (size_t)K, st)) return rc;
      TR_HIP(hipMemsetAsync(ent, 0, sizeof(dint_traffic_key) * K, st));
      TR_HIP(hipMemsetAsync(sreq, 0, 4 * K, st));
      TR_HIP(hipMemsetAsync(srej, 0, 4 * K, st));
      hipLaunchKernelGGL(k_tr_key_reduce, dim3(tr_blocks(K)), dim3(TRK_TB), 0, st, (const uint64_t *)key, (const uint32_t *)meta, perm, (const uint32_t *)head,
                         (const uint32_t *)seg, (uint32_t)K, ent, sreq, srej);
      TR_HIP(hipGetLastError());
      uint32_t d32 = 0;
      TR_HIP(hipMemcpyAsync(&d32, seg + (K - 1), 4, hipMemcpyDeviceToHost, st));
      TR_HIP(hipStreamSynchronize(st));  // (2) the distinct keys
      D = d32;
      if (D == 0 || D > K) {
        dint_set_last_error("traffic report: the runs do not add up to the keyed requests (an internal error)");
        return DINT_EHIP;
      }
      // ---- per key, per unit, per lock slot.  From here on the first stage's arrays are dead: the sorted group words take key_s,
      // their key numbers idx1, heads and scan the arrays of the same name, the sorted counts and the order idx2 and idx1; idx0 is
      // 0, 1, 2 ..: the key numbers
      const uint32_t slots = tr_has_slots(g.workload) ? 1u : 0u;
      hipLaunchKernelGGL(k_tr_key_stats, dim3(tr_blocks(D)), dim3(TRK_TB), 0, st, (const dint_traffic_key *)ent, (const uint32_t *)sreq, (uint32_t)D, g, slots, ukey,
                         lkey, rk, jk, s.words);
      for (uint32_t slot = 0; slot <= slots; slot++) {
        if (int rc = tr_sort(tmp, l.tmp_bytes, (const uint64_t *)(slot ? lkey : ukey), key_s, (const uint32_t *)idx0, idx1, (size_t)D, 0u, 64u, st)) return rc;
        hipLaunchKernelGGL(k_tr_group_heads, dim3(tr_blocks(D)), dim3(TRK_TB), 0, st, (const uint64_t *)key_s, (uint32_t)D, head);
        if (int rc = tr_scan(tmp, l.tmp_bytes, (const uint32_t *)head, seg, (size_t)D, st)) return rc;
        TR_HIP(hipMemsetAsync(gcnt, 0, 12 * D, st));
        hipLaunchKernelGGL(k_tr_group_reduce, dim3(tr_blocks(D)), dim3(TRK_TB), 0, st, (const uint64_t *)key_s, (const uint32_t *)idx1, (const uint32_t *)head,
                           (const uint32_t *)seg, (uint32_t)D, (const dint_traffic_key *)ent, (const uint32_t *)sreq, (const uint32_t *)srej, slot, gcnt, gk_out);
        hipLaunchKernelGGL(k_tr_group_stats, dim3(tr_blocks(D)), dim3(TRK_TB), 0, st, (const uint32_t *)gcnt, (const uint32_t *)seg, (uint32_t)D, slot, s.words);
        if (!slot) hipLaunchKernelGGL(k_tr_max_unit, dim3(1), dim3(64), 0, st, (const uint64_t *)gk_out, s.words);
      }
      // ---- the two lists
      if (top_k) {
        for (uint32_t which = 0; which < 2; which++) {
          if (which && !d_rep) break;
          if (int rc = tr_sort(tmp, l.tmp_bytes, (const uint32_t *)(which ? jk : rk), idx2, (const uint32_t *)idx0, idx1, (size_t)D, 0u, 25u, st)) return rc;
          hipLaunchKernelGGL(k_tr_emit, dim3(tr_blocks(std::min<uint64_t>(top_k, D))), dim3(TRK_TB), 0, st, (const dint_traffic_key *)ent, (const uint32_t *)idx1,
                             (uint32_t)D, top_k, which ? (const unsigned long long *)(s.words + TRX_NREJ) : nullptr, s.top + (size_t)which * DINT_TRAFFIC_MAX_TOP);
        }
      }
      TR_HIP(hipGetLastError());
      TR_HIP(hipMemcpyAsync(h.data(), s.words, (size_t)TRX_WORDS_END * 8, hipMemcpyDeviceToHost, st));
      TR_HIP(hipStreamSynchronize(st));  // (3) the result (the lists are copied behind it: their lengths are known now)
      nrej = d_rep ? h[TRX_NREJ] : 0;
    }
  }
  const uint64_t n_req = std::min<uint64_t>(top_k, D), n_rej = std::min<uint64_t>(top_k, nrej);
  std::vector<dint_traffic_key> lists(n_req + n_rej);
  if (n_req) TR_HIP(hipMemcpy(lists.data(), s.top, n_req * sizeof(dint_traffic_key), hipMemcpyDeviceToHost));
  if (n_rej) TR_HIP(hipMemcpy(lists.data() + n_req, s.top + DINT_TRAFFIC_MAX_TOP, n_rej * sizeof(dint_traffic_key), hipMemcpyDeviceToHost));
  h[TR_W_N] = n;
  h[TR_W_DKEYS] = D;
  h[TR_W_N_BY_REQ] = n_req;
  h[TR_W_N_BY_REJ] = n_rej;
  h[TR_W_TEMP] = temp;
  memcpy(out, h.data(), sizeof *out);
  if (n_req) memcpy(by_requests, lists.data(), n_req * sizeof(dint_traffic_key));
  if (n_rej) memcpy(by_rejects, lists.data() + n_req, n_rej * sizeof(dint_traffic_key));
  return 0;
}

// ---- the host form (include/dint_driver.h): the same traffic_report.h rule over a batch in host memory -------------------------
extern "C" int dint_traffic_report_host(uint32_t workload, uint64_t n_slots, uint64_t n_rows, uint32_t flags, const void *reqs, const void *replies, uint64_t n,
                                        uint32_t top_k, struct dint_traffic_report *out, dint_traffic_key *by_requests, dint_traffic_key *by_rejects) {
  tr_geom g;
  if (workload == DINT_WL_LOG) {
    dint_set_last_error("a log_server batch has no keys to report");
    return DINT_ESTATE;
  }
  if (!out || (n && !reqs) || (top_k && (!by_requests || !by_rejects)) || top_k > DINT_TRAFFIC_MAX_TOP || n > DINT_TRAFFIC_MAX_N || (n && replies == reqs) ||
      !dint_traffic_geom(workload, n_slots, n_rows, flags, &g)) {
    dint_set_last_error("traffic report: out, n <= 2^24 requests, top_k <= 4096 with both lists, replies that are not the request array, a keyed workload");
    return DINT_EINVAL;
  }
  struct item {
    uint64_t key;
    uint32_t table, meta, index;
  };
  struct group {
    uint64_t word;
    uint32_t req, rej;
  };
  try {
    const tr_format f = tr_format_of(workload);
    std::vector<uint64_t> w(TR_WORDS, 0);
    std::vector<item> items;
    const uint8_t *rq = (const uint8_t *)reqs, *rp = (const uint8_t *)replies;
    for (uint64_t i = 0; i < n; i++) {
      uint64_t key;
      uint32_t t, y, yr;
      const uint8_t *p = rq + i * f.msg;
      const uint32_t m = tr_decode(g, f, p, rp ? rp + i * f.msg : p, rp != nullptr, &key, &t, &y, &yr);
      if (t >= g.n_tables) {
        w[TR_W_BAD_TABLE]++;
        continue;
      }
      w[TR_W_REQ_TYPES + t * TR_TYPE_BINS + tr_type_bin(y)]++;
      if (rp) w[TR_W_REP_TYPES + t * TR_TYPE_BINS + tr_type_bin(yr)]++;
      const uint32_t c = m & TR_M_CLASS;
      if (c == TR_LOG) {
        w[TR_W_LOG]++;
        continue;
      }
      w[TR_W_KEYED]++;
      w[c == TR_OTHER ? TR_W_OTHERS : TR_W_READS + c]++;
      if (m & TR_M_REJECT) w[TR_W_REJECTS]++;
      if (m & TR_M_MISS) w[TR_W_MISSES]++;
      items.push_back({key, t, m, (uint32_t)i});
    }
    std::sort(items.begin(), items.end(), [](const item &a, const item &b) {
      return a.table != b.table ? a.table < b.table : a.key != b.key ? a.key < b.key : a.index < b.index;
    });
    std::vector<dint_traffic_key> ent;
    std::vector<group> units, slots;
    for (size_t j = 0; j < items.size();) {
      dint_traffic_key e;
      memset(&e, 0, sizeof e);
      e.key = items[j].key;
      e.table = items[j].table;
      e.first_index = items[j].index;
      uint32_t sreq = 0, srej = 0;
      for (; j < items.size() && items[j].key == e.key && items[j].table == e.table; j++) {
        const uint32_t m = items[j].meta, c = m & TR_M_CLASS;
        e.requests++;
        if (c == TR_READ) e.reads++;
        if (c == TR_LOCK) e.locks++;
        if (c == TR_UNLOCK) e.unlocks++;
        if (c == TR_WRITE) e.writes++;
        if (m & TR_M_REJECT) e.rejects++;
        if (m & TR_M_MISS) e.misses++;
        if (m & TR_M_SLOT) {
          sreq++;
          if (m & TR_M_REJECT) srej++;
        }
      }
      ent.push_back(e);
      w[TR_W_KEY_HIST + tr_count_bin(e.requests)]++;
      w[TR_W_MAX_KEY] = std::max<uint64_t>(w[TR_W_MAX_KEY], e.requests);
      units.push_back({tr_unit(g, e.table, e.key), e.requests, e.rejects});
      if (tr_has_slots(workload) && sreq) slots.push_back({tr_slot(g, e.table, e.key), sreq, srej});
    }
    w[TR_W_N] = n;
    w[TR_W_DKEYS] = ent.size();
    for (int slot = 0; slot < 2; slot++) {
      std::vector<group> &v = slot ? slots : units;
      std::sort(v.begin(), v.end(), [](const group &a, const group &b) { return a.word < b.word; });
      for (size_t j = 0; j < v.size();) {
        const uint64_t word = v[j].word;
        uint64_t keys = 0, req = 0, rej = 0;
        for (; j < v.size() && v[j].word == word; j++) {
          keys++;
          req += v[j].req;
          rej += v[j].rej;
        }
        w[slot ? TR_W_DSLOTS : TR_W_DUNITS]++;
        if (keys >= 2) {
          w[slot ? TR_W_SH_SLOTS : TR_W_SH_UNITS]++;
          w[slot ? TR_W_SH_SLOT_REQ : TR_W_SH_UNIT_REQ] += req;
          w[slot ? TR_W_SH_SLOT_REJ : TR_W_SH_UNIT_REJ] += rej;
        }
        if (!slot) {
          w[TR_W_UNIT_HIST + tr_count_bin((uint32_t)req)]++;
          if (req > w[TR_W_MAX_UNIT_REQ]) {  // (ascending words: the first to attain it stays)
            w[TR_W_MAX_UNIT_REQ] = req;
            w[TR_W_MAX_UNIT] = word & ((1ull << TR_GROUP_TABLE_SHIFT) - 1);
            w[TR_W_MAX_UNIT_TABLE] = word >> TR_GROUP_TABLE_SHIFT;
          }
        }
      }
    }
    std::vector<dint_traffic_key> top[2];
    for (int which = 0; which < 2 && top_k; which++) {
      std::vector<dint_traffic_key> v;
      for (const dint_traffic_key &e : ent)
        if (!which || e.rejects) v.push_back(e);
      std::stable_sort(v.begin(), v.end(), [which](const dint_traffic_key &a, const dint_traffic_key &b) {
        return which ? a.rejects > b.rejects : a.requests > b.requests;
      });
      if (v.size() > top_k) v.resize(top_k);
      top[which].swap(v);
    }
    w[TR_W_N_BY_REQ] = top[0].size();
    w[TR_W_N_BY_REJ] = top[1].size();
    memcpy(out, w.data(), sizeof *out);
    if (!top[0].empty()) memcpy(by_requests, top[0].data(), top[0].size() * sizeof(dint_traffic_key));
    if (!top[1].empty()) memcpy(by_rejects, top[1].data(), top[1].size() * sizeof(dint_traffic_key));
  } catch (const std::bad_alloc &) {
    dint_set_last_error("out of host memory");
    return DINT_ENOMEM;
  }
  return 0;
}
