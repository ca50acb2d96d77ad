// k_block.hip -- two replicas compared block by block, and only the blocks that differ shipped (include/dint_abi.h
// dint_state_block_digest / dint_state_block_select / dint_state_block_rows / dint_state_block_diff, driven by engine.hip; the
// rule lives in state_block.h, which the host forms at the end of this file share).  Not on a request's path.
//
//   k_block_digest       a table's INLINE entries are contiguous in local-bucket order, so a chunk of 64 buckets is one range:
//                        a workgroup streams chunk after chunk as 16-byte vectors through LDS (k_state.hip k_state_digest's
//                        layout), one thread hashes one slot from LDS, and only the lane of a bucket whose chain leaves its
//                        inline entry walks on into the pool (state_dev.h sd_bucket under state_image.h si_chain_walk) and
//                        hashes what it finds there from HBM.  An inline entry counts iff its chain holds it.  One partial
//                        {rows, sum, xr, 0} per chunk: with B = 64 that IS the block's digest and goes to the caller's array
//   k_block_merge        B > 64: a wave per block adds up the block's chunks.  No atomics; integer arithmetic, any order
//   k_block_select       ONE workgroup of 1,024 compares the two arrays, 1,024 blocks a round, and writes the ids of the blocks
//                        whose 32 bytes differ in ascending order (a scan per round, a running base): no scratch but one word
//   k_block_ids          the id list checked (strictly ascending, in range); per id its bucket count, then state_dev.h's scan:
//                        LANES = the buckets of the listed blocks laid end to end
//   k_block_rows_count   one lane per bucket of the listed blocks: its visible rows; per workgroup one count, then the scan
//   k_block_rows_write   (launched when the host has read the total) the count again, a scan in the workgroup, the records
//   k_block_diff_check   one lane per row of the list: table, home and order; the first and the last row of a bucket's run store
//                        where the run starts and ends at the bucket's lane (a neighbour compare, no search per lane)
//   k_block_diff_count / _write   as the rows', over state_sync.h ss_bucket_diff(the bucket's run, the replica's chain)
// A kernel that finds the `bad` word set does nothing; the host reads it with the totals and writes nothing for a bad list.
// Every chain walk counts to KV_MAX_CHAIN and checks its links; no content of a table, an id list or a row list makes a kernel
// read or write outside the tables, the lists and the scratch, or loop without bound.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/dint_abi.h"
#include "../../include/dint_driver.h"
#include "dint_kernels.h"
#include "dint_kv.h"
#include "state_block.h"
#include "state_dev.h"
#include "state_sync.h"

#define BK_TB SD_TB
#define BK_LDS_PAD 16u            // bytes between entries in LDS (k_state.hip SS_LDS_PAD)
#define BK_DIGEST_GRID 2048u      // workgroups per table at most; they stride over the chunks

static_assert(BK_TB == 4 * BK_CHUNK, "the digest hashes one slot per thread");
static_assert(sizeof(dint_block_digest) == 32 && sizeof(dint_block_stats) == 64, "the ABI's block structs");
static_assert(BK_MAX_RUN == SS_WALK_BOUND && BK_MAX_RUN < 65536u, "a bucket's counts by kind fit 16 bits each");

struct bk_dev_ld {  // a row list in device memory: 8-byte aligned
  __device__ static inline uint32_t u32(const uint8_t *p) { return *(const uint32_t *)p; }
  __device__ static inline uint64_t u64(const uint8_t *p) { return *(const uint64_t *)p; }
};

// ------------------------------------------------------------------------------------------------------ digest
template <uint32_t VS>
__device__ static inline uint64_t bk_hash_hbm(const uint8_t *e, uint32_t s, uint32_t table) {
  const uint8_t *val = e + KV_VAL_OFF + s * VS;
  return ss_row_hash(KV_LD(uint64_t, e + 8 * s), KV_LD(uint32_t, e + 32 + 4 * s), table, VS,
                     [val](uint32_t k) { return KV_LD(uint64_t, val + 8 * k); });
}

// out[4 c ..] = {rows, sum, xr, 0} of chunk c of this table
template <uint32_t STRIDE>
__global__ void __launch_bounds__(BK_TB) k_block_digest(kv_tab t, uint32_t table, uint32_t n_chunks, unsigned long long *__restrict__ out) {
  constexpr uint32_t VPE = STRIDE / 16;               // vectors per entry
  constexpr uint32_t LSTRIDE = STRIDE + BK_LDS_PAD;   // an entry's distance in LDS
  constexpr uint32_t VS = STRIDE == 256 ? 40u : 8u;
  constexpr uint32_t VPT = BK_CHUNK * VPE / BK_TB;    // vectors per thread and chunk
  __shared__ sd_v4 Lv[BK_CHUNK * LSTRIDE / 16];
  __shared__ uint64_t red[BK_TB / 64][3];
  const uint8_t *L = (const uint8_t *)Lv;
  const uint32_t tid = threadIdx.x;
  const uint64_t n_vec = t.n_local * VPE;  // (the inline entries only: the pool behind them is reached through the chains)
  const KV_G(sd_v4) *src = (const KV_G(sd_v4) *)t.entries;
  for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {  // (uniform in the workgroup)
    const uint64_t v0 = (uint64_t)c * BK_CHUNK * VPE;
    sd_v4 v[VPT];
#pragma unroll
    for (uint32_t k = 0; k < VPT; k++) {
      const uint64_t g = v0 + k * BK_TB + tid;
      v[k] = g < n_vec ? __builtin_nontemporal_load(src + g) : (sd_v4)(0u);
    }
#pragma unroll
    for (uint32_t k = 0; k < VPT; k++) {
      const uint32_t i = k * BK_TB + tid;
      Lv[(i / VPE) * (LSTRIDE / 16) + (i % VPE)] = v[k];
    }
    __syncthreads();
    const uint8_t *e = L + (tid >> 2) * LSTRIDE;
    const uint32_t s = tid & 3;
    const sd_v4 lv = *(const sd_v4 *)(e + 16 * SI_LINK_VEC);  // {validw, next, head, lockw}
    const bool inl_first = lv.z == KV_INLINE;
    ss_digest d = {0, 0, 0};
    if (inl_first && ((lv.x >> (8 * s)) & 0xFFu)) {
      const uint64_t *val = (const uint64_t *)(e + KV_VAL_OFF + s * VS);
      ss_digest_add(d, ss_row_hash(*(const uint64_t *)(e + 8 * s), *(const uint32_t *)(e + 32 + 4 * s), table, VS,
                                   [val](uint32_t k) { return val[k]; }));
    }
    if (s == 0 && lv.z != KV_NULL && !(inl_first && lv.y == KV_NULL)) {  // (a bucket beyond the table came in as zeros: head 0)
      const uint64_t b = (uint64_t)c * BK_CHUNK + (tid >> 2);
      const sd_bucket ch = {t, b, lv};
      (void)si_chain_walk(lv.z, ch, [&](uint32_t, uint32_t link, uint32_t validw) {
        if (link == KV_INLINE && inl_first) return true;  // (its four slots are the four threads')
        const uint8_t *h = kv_entry_ptr(t, b, link);
#pragma unroll
        for (uint32_t i = 0; i < 4; i++)
          if ((validw >> (8 * i)) & 0xFFu) ss_digest_add(d, bk_hash_hbm<VS>(h, i, table));
        return true;
      });
    }
    const ss_digest w = ss_block_digest(red, d);  // (one barrier: the tile has been read by then)
    if (tid == 0) {
      unsigned long long *o = out + 4 * (size_t)c;
      o[0] = w.rows; o[1] = w.sum; o[2] = w.xr; o[3] = 0;
    }
    // (red is written again only behind the next round's barrier, which thread 0 reaches after it has read red)
  }
}

struct bk_merge_arg {
  bk_geom g;
  uint64_t chunk_at[BK_MAX_TABLES];  // a table's first chunk in part
};
// out[4 id ..] = the chunks of block id added up; a wave per block
__global__ void __launch_bounds__(BK_TB) k_block_merge(const unsigned long long *__restrict__ part, bk_merge_arg a, unsigned long long *__restrict__ out) {
  const uint64_t id64 = (uint64_t)blockIdx.x * (BK_TB / 64) + (threadIdx.x >> 6);
  if (id64 >= bk_blocks(a.g)) return;  // (uniform in the wave)
  const uint32_t id = (uint32_t)id64, lane = threadIdx.x & 63;
  const bk_block b = bk_locate(a.g, id);
  const uint64_t c0 = a.chunk_at[b.table] + b.first / BK_CHUNK, nc = (b.count + BK_CHUNK - 1) / BK_CHUNK;
  ss_digest d = {0, 0, 0};
  for (uint64_t k = lane; k < nc; k += 64) {
    const unsigned long long *p = part + 4 * (c0 + k);
    ss_digest_merge(d, ss_digest{p[0], p[1], p[2]});
  }
  d.rows = sd_wave_sum_u64(d.rows);
  d.sum = sd_wave_sum_u64(d.sum);
  d.xr = sd_wave_xor_u64(d.xr);
  if (lane == 0) {
    unsigned long long *o = out + 4 * (size_t)id;
    o[0] = d.rows; o[1] = d.sum; o[2] = d.xr; o[3] = 0;
  }
}

// ------------------------------------------------------------------------------------------------------ select
__global__ void __launch_bounds__(1024) k_block_select(const unsigned long long *__restrict__ a, const unsigned long long *__restrict__ b, uint32_t n,
                                                       uint32_t *__restrict__ ids, uint64_t cap, unsigned long long *total) {
  __shared__ uint32_t wsum[16];
  const uint32_t tid = threadIdx.x;
  uint64_t base = 0;
  for (uint64_t i0 = 0; i0 < n; i0 += 1024) {  // (uniform in the workgroup)
    const uint64_t i = i0 + tid;
    uint32_t differs = 0;
    if (i < n) differs = ((a[4 * i] ^ b[4 * i]) | (a[4 * i + 1] ^ b[4 * i + 1]) | (a[4 * i + 2] ^ b[4 * i + 2]) | (a[4 * i + 3] ^ b[4 * i + 3])) != 0;
    uint32_t tot;
    uint32_t before = wave_excl_scan_u32(differs, &tot);
    if ((tid & 63) == 0) wsum[tid >> 6] = tot;
    __syncthreads();
    uint32_t all = 0;
    for (uint32_t w = 0; w < 16; w++) {
      if (w < (tid >> 6)) before += wsum[w];
      all += wsum[w];
    }
    if (differs && base + before < cap) ids[base + before] = (uint32_t)i;
    base += all;
    __syncthreads();
  }
  if (tid == 0) *total = base;
}

// ------------------------------------------------------------------------------------------------------ the listed blocks' lanes
__global__ void __launch_bounds__(BK_TB) k_block_ids(const uint32_t *__restrict__ ids, uint32_t n, bk_geom g, uint32_t *__restrict__ cnt, uint32_t *bad) {
  const uint64_t j = (uint64_t)blockIdx.x * BK_TB + threadIdx.x;
  if (j >= n) return;
  const uint32_t id = ids[j];
  const bool ok = id < bk_blocks(g) && (j == 0 || ids[j - 1] < id);
  cnt[j] = ok ? (uint32_t)bk_locate(g, id).count : 0u;
  if (!ok) atomicOr(bad, (uint32_t)BK_BAD_IDS);
}
struct bk_lanes {
  const uint32_t *ids;
  const uint64_t *off;           // the exclusive scan of the listed blocks' bucket counts
  uint32_t n_ids;
  const unsigned long long *n;   // their sum
};
// lane l's bucket; only with a good id list
__device__ static inline bool bk_lane_bucket(const bk_lanes &ln, const bk_geom &g, uint64_t l, uint32_t &table, uint64_t &bucket) {
  if (ln.n_ids == 0 || l >= *ln.n) return false;
  uint32_t lo = 0, hi = ln.n_ids;
  while (hi - lo > 1) {  // the last listed block that starts at or before l
    const uint32_t mid = lo + (hi - lo) / 2;
    if (ln.off[mid] <= l) lo = mid;
    else hi = mid;
  }
  const bk_block b = bk_locate(g, ln.ids[lo]);
  const uint64_t o = l - ln.off[lo];
  if (o >= b.count) return false;
  table = b.table;
  bucket = b.first + o;
  return true;
}

// ------------------------------------------------------------------------------------------------------ rows
__device__ static inline uint32_t bk_visible_count(const ss_chain &ch) {
  uint32_t c = 0, steps = 0;
  for (uint64_t p = ch.begin(); ch.ok(p) && steps < SS_WALK_BOUND; p = ch.next(p), steps++) c += ch.same(ch.find(ch.key(p)), p);
  return c;
}
__global__ void __launch_bounds__(BK_TB) k_block_rows_count(const kv_dev *__restrict__ kv, bk_geom g, bk_lanes ln, uint32_t *__restrict__ cnt, const uint32_t *bad) {
  __shared__ uint32_t red[BK_TB / 64][1];
  uint32_t c = 0, table;
  uint64_t bucket;
  if (*bad == 0 && bk_lane_bucket(ln, g, (uint64_t)blockIdx.x * BK_TB + threadIdx.x, table, bucket)) c = bk_visible_count(ss_chain{kv->tab[table], bucket});
  sd_block_sum(red, {c});
  if (threadIdx.x == 0) cnt[blockIdx.x] = sd_block_total(red, 0);
}
template <uint32_t VS>
__global__ void __launch_bounds__(BK_TB) k_block_rows_write(const kv_dev *__restrict__ kv, bk_geom g, bk_lanes ln, const uint64_t *__restrict__ off, uint8_t *out,
                                                            uint64_t cap) {
  __shared__ uint32_t red[BK_TB / 64];
  const uint64_t at0 = off[blockIdx.x];
  if (at0 >= cap) return;  // (workgroup-uniform)
  uint32_t c = 0, table = 0;
  uint64_t bucket = 0;
  const bool mine = bk_lane_bucket(ln, g, (uint64_t)blockIdx.x * BK_TB + threadIdx.x, table, bucket);
  if (mine) c = bk_visible_count(ss_chain{kv->tab[table], bucket});
  const uint32_t before = sd_block_excl_scan(red, c);
  if (c == 0 || at0 + before >= cap) return;
  const ss_chain ch = {kv->tab[table], bucket};
  ss_write_emit<VS> em = {out, at0 + before, cap, table};
  uint32_t steps = 0;
  for (uint64_t p = ch.begin(); ch.ok(p) && steps < SS_WALK_BOUND; p = ch.next(p), steps++)
    if (ch.same(ch.find(ch.key(p)), p)) em(SS_ONLY_A, ch, p);
}

// ------------------------------------------------------------------------------------------------------ diff
__device__ static inline bk_place bk_dev_place(const uint8_t *r, const bk_geom &g, const kv_dev *kv) {
  return bk_row_place<bk_dev_ld>(r, g, kv->shard_index, kv->shard_count,
                                 [kv](uint64_t key, uint32_t table) { return dint_fastmod(dint_hash_key(key), kv->mod[table]); });
}
__global__ void __launch_bounds__(BK_TB) k_block_diff_check(const uint8_t *__restrict__ rec, uint32_t n, const kv_dev *__restrict__ kv, bk_geom g, bk_lanes ln,
                                                            uint32_t *__restrict__ run_lo, uint32_t *__restrict__ run_hi, uint64_t run_cap, uint32_t *bad) {
  const uint64_t i = (uint64_t)blockIdx.x * BK_TB + threadIdx.x;
  if (i >= n || (*(volatile uint32_t *)bad & BK_BAD_IDS)) return;
  const bk_place me = bk_dev_place(rec + i * 64, g, kv);
  uint32_t b = me.bad;
  uint64_t lane = ~0ull;
  if (!b) {
    const uint32_t j = bk_find_id(ln.ids, ln.n_ids, bk_id_of(g, me.table, me.bucket));
    if (j == ln.n_ids) b = BK_BAD_HOME;
    else lane = ln.off[j] + (me.bucket & ((1ull << g.shift) - 1));
  }
  bool head = true, tail = true;
  if (!b && i > 0) {
    const bk_place prev = bk_dev_place(rec + (i - 1) * 64, g, kv);
    if (!prev.bad) {  // (a bad neighbour reports itself)
      if (prev.order() > me.order()) b = BK_BAD_ORDER;
      head = prev.order() != me.order();
    }
  }
  if (!b && i + 1 < n) {
    const bk_place next = bk_dev_place(rec + (i + 1) * 64, g, kv);
    tail = next.bad || next.order() != me.order();
  }
  if (b) {
    atomicOr(bad, b);
  } else if (lane < run_cap) {
    if (head) run_lo[lane] = (uint32_t)i;
    if (tail) run_hi[lane] = (uint32_t)i + 1u;
  }
}
// lane l's run, or an empty one
__device__ static inline bk_run<bk_dev_ld> bk_lane_run(const uint8_t *rec, const uint32_t *run_lo, const uint32_t *run_hi, uint64_t l, uint32_t n_rows, uint32_t *bad) {
  uint32_t lo = run_lo[l], hi = run_hi[l];
  if (lo > hi || hi > n_rows) lo = hi = 0;  // (never in a list that passed the check)
  if (hi - lo > BK_MAX_RUN) {
    atomicOr(bad, (uint32_t)BK_BAD_RUN);
    lo = hi = 0;
  }
  return bk_run<bk_dev_ld>{rec + (size_t)lo * 64, hi - lo};
}
template <uint32_t VS>
__global__ void __launch_bounds__(BK_TB) k_block_diff_count(const uint8_t *__restrict__ rec, uint32_t n_rows, const kv_dev *__restrict__ kv, bk_geom g, bk_lanes ln,
                                                            const uint32_t *__restrict__ run_lo, const uint32_t *__restrict__ run_hi, uint32_t *__restrict__ cnt,
                                                            unsigned long long *stats, uint32_t *bad) {
  __shared__ uint32_t red[BK_TB / 64][4];
  const uint64_t l = (uint64_t)blockIdx.x * BK_TB + threadIdx.x;
  uint64_t packed = 0, bucket;
  uint32_t table;
  if ((*(volatile uint32_t *)bad & ~(uint32_t)BK_BAD_RUN) == 0 && bk_lane_bucket(ln, g, l, table, bucket)) {
    const bk_run<bk_dev_ld> a = bk_lane_run(rec, run_lo, run_hi, l, n_rows, bad);
    const ss_chain cb = {kv->tab[table], bucket};
    ss_count_emit em;
    ss_bucket_diff(a, cb, VS, SS_WALK_BOUND, em);
    packed = em.packed;
  }
  sd_block_sum(red, {(uint32_t)packed & 0xFFFFu, (uint32_t)(packed >> 16) & 0xFFFFu, (uint32_t)(packed >> 32) & 0xFFFFu, (uint32_t)(packed >> 48)});
  if (threadIdx.x < 4) {
    const uint32_t s = sd_block_total(red, threadIdx.x);
    if (s) atomicAdd(stats + threadIdx.x, (unsigned long long)s);
    red[0][threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) cnt[blockIdx.x] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
}
template <uint32_t VS>
__global__ void __launch_bounds__(BK_TB) k_block_diff_write(const uint8_t *__restrict__ rec, uint32_t n_rows, const kv_dev *__restrict__ kv, bk_geom g, bk_lanes ln,
                                                            const uint32_t *__restrict__ run_lo, const uint32_t *__restrict__ run_hi,
                                                            const uint64_t *__restrict__ off, uint8_t *out, uint64_t cap, uint32_t *bad) {
  __shared__ uint32_t red[BK_TB / 64];
  const uint64_t at0 = off[blockIdx.x];
  if (at0 >= cap) return;  // (workgroup-uniform)
  const uint64_t l = (uint64_t)blockIdx.x * BK_TB + threadIdx.x;
  uint32_t table = 0, mine = 0;
  uint64_t bucket = 0;
  const bool have = bk_lane_bucket(ln, g, l, table, bucket);
  bk_run<bk_dev_ld> a = {rec, 0};
  if (have) {
    a = bk_lane_run(rec, run_lo, run_hi, l, n_rows, bad);
    const ss_chain cb = {kv->tab[table], bucket};
    ss_count_emit em;
    ss_bucket_diff(a, cb, VS, SS_WALK_BOUND, em);
    mine = (uint32_t)(em.packed & 0xFFFFu) + (uint32_t)((em.packed >> 16) & 0xFFFFu) + (uint32_t)((em.packed >> 32) & 0xFFFFu) + (uint32_t)(em.packed >> 48);
  }
  const uint32_t before = sd_block_excl_scan(red, mine);
  if (mine == 0 || at0 + before >= cap) return;
  const ss_chain cb = {kv->tab[table], bucket};
  ss_write_emit<VS> em = {out, at0 + before, cap, table};
  ss_bucket_diff(a, cb, VS, SS_WALK_BOUND, em);
}

// ------------------------------------------------------------------------------------------------------ host side
bool dint_block_geom(const dint_kv &kv, uint64_t block_buckets, bk_geom *g) {
  uint64_t n_local[BK_MAX_TABLES] = {0, 0, 0, 0, 0};
  for (uint32_t t = 0; t < kv.n_tables; t++) n_local[t] = kv.h.tab[t].n_local;
  return bk_geom_make(*g, kv.n_tables, n_local, block_buckets);
}
uint64_t dint_block_chunks(const dint_kv &kv) {
  uint64_t n = 0;
  for (uint32_t t = 0; t < kv.n_tables; t++) n += bk_table_chunks(kv.h.tab[t].n_local);
  return n;
}

// s.part holds dint_block_chunks(kv) partials (not needed for B = 64); d_out bk_blocks(g) digests
void dint_launch_block_digest(const dint_kv &kv, const bk_geom &g, dint_block_scratch s, void *d_out, hipStream_t st) {
  const bool direct = g.shift == 6;
  bk_merge_arg a;
  a.g = g;
  uint64_t at = 0;
  for (uint32_t t = 0; t < BK_MAX_TABLES; t++) {
    a.chunk_at[t] = at;
    if (t < kv.n_tables) at += bk_table_chunks(kv.h.tab[t].n_local);
  }
  for (uint32_t t = 0; t < kv.n_tables; t++) {
    const kv_tab &tb = kv.h.tab[t];
    const uint32_t nc = (uint32_t)bk_table_chunks(tb.n_local);
    if (nc == 0) continue;
    unsigned long long *o = direct ? (unsigned long long *)d_out + 4 * (size_t)g.first[t] : s.part + 4 * a.chunk_at[t];
    const uint32_t grid = std::min<uint32_t>(nc, BK_DIGEST_GRID);
    if (tb.stride == 256) hipLaunchKernelGGL(k_block_digest<256>, dim3(grid), dim3(BK_TB), 0, st, tb, t, nc, o);
    else hipLaunchKernelGGL(k_block_digest<128>, dim3(grid), dim3(BK_TB), 0, st, tb, t, nc, o);
  }
  if (!direct && bk_blocks(g))
    hipLaunchKernelGGL(k_block_merge, dim3((bk_blocks(g) + BK_TB / 64 - 1) / (BK_TB / 64)), dim3(BK_TB), 0, st, (const unsigned long long *)s.part, a,
                       (unsigned long long *)d_out);
}

static bk_lanes bk_lanes_of(const dint_block_scratch &s, const void *d_ids, uint32_t n_ids) {
  return bk_lanes{(const uint32_t *)d_ids, (const uint64_t *)s.id_off, n_ids, s.words + DINT_BLOCK_LANES_AT};
}
static uint32_t bk_grid(uint64_t n) { return (uint32_t)((n + BK_TB - 1) / BK_TB); }

// the words cleared, the id list checked and scanned: s.words[DINT_BLOCK_LANES_AT] = the lanes, (u32) s.words[DINT_BLOCK_BAD_AT] |= BK_BAD_IDS
static void bk_launch_ids(const bk_geom &g, const void *d_ids, uint32_t n_ids, dint_block_scratch s, hipStream_t st) {
  (void)hipMemsetAsync(s.words, 0, DINT_BLOCK_WORDS * sizeof(unsigned long long), st);
  hipLaunchKernelGGL(k_block_ids, dim3(bk_grid(n_ids)), dim3(BK_TB), 0, st, (const uint32_t *)d_ids, n_ids, g, s.id_cnt, (uint32_t *)(s.words + DINT_BLOCK_BAD_AT));
  sd_launch_scan((const uint32_t *)s.id_cnt, n_ids, s.id_off, s.words + DINT_BLOCK_LANES_AT, st);
}

// n_ids > 0; `lanes` = what the caller sized the scratch for (dint_block_lanes_max).  Afterwards s.words[DINT_BLOCK_TOTAL_AT] = the records
void dint_launch_block_rows_count(const dint_kv &kv, const bk_geom &g, const void *d_ids, uint32_t n_ids, uint64_t lanes, dint_block_scratch s, hipStream_t st) {
  bk_launch_ids(g, d_ids, n_ids, s, st);
  const uint32_t nb = bk_grid(lanes);
  hipLaunchKernelGGL(k_block_rows_count, dim3(nb), dim3(BK_TB), 0, st, (const kv_dev *)kv.d_dev, g, bk_lanes_of(s, d_ids, n_ids), s.blk_cnt,
                     (const uint32_t *)(s.words + DINT_BLOCK_BAD_AT));
  sd_launch_scan((const uint32_t *)s.blk_cnt, nb, s.blk_off, s.words + DINT_BLOCK_TOTAL_AT, st);
}
void dint_launch_block_rows_write(const dint_kv &kv, const bk_geom &g, const void *d_ids, uint32_t n_ids, uint64_t lanes, dint_block_scratch s, void *d_records,
                                  uint64_t cap, hipStream_t st) {
  const uint32_t nb = bk_grid(lanes);
  if (kv.val_size == 40)
    hipLaunchKernelGGL(k_block_rows_write<40>, dim3(nb), dim3(BK_TB), 0, st, (const kv_dev *)kv.d_dev, g, bk_lanes_of(s, d_ids, n_ids), (const uint64_t *)s.blk_off,
                       (uint8_t *)d_records, cap);
  else
    hipLaunchKernelGGL(k_block_rows_write<8>, dim3(nb), dim3(BK_TB), 0, st, (const kv_dev *)kv.d_dev, g, bk_lanes_of(s, d_ids, n_ids), (const uint64_t *)s.blk_off,
                       (uint8_t *)d_records, cap);
}

// n_ids > 0.  Afterwards s.words[0 .. 3] = the records by kind, [DINT_BLOCK_TOTAL_AT] their number, [DINT_BLOCK_BAD_AT] what the checks found
void dint_launch_block_diff_count(const dint_kv &kv, const bk_geom &g, const void *d_ids, uint32_t n_ids, uint64_t lanes, const void *d_rows, uint32_t n_rows,
                                  dint_block_scratch s, hipStream_t st) {
  bk_launch_ids(g, d_ids, n_ids, s, st);
  (void)hipMemsetAsync(s.run_lo, 0, lanes * sizeof(uint32_t), st);
  (void)hipMemsetAsync(s.run_hi, 0, lanes * sizeof(uint32_t), st);
  uint32_t *bad = (uint32_t *)(s.words + DINT_BLOCK_BAD_AT);
  const bk_lanes ln = bk_lanes_of(s, d_ids, n_ids);
  if (n_rows)
    hipLaunchKernelGGL(k_block_diff_check, dim3(bk_grid(n_rows)), dim3(BK_TB), 0, st, (const uint8_t *)d_rows, n_rows, (const kv_dev *)kv.d_dev, g, ln, s.run_lo,
                       s.run_hi, lanes, bad);
  const uint32_t nb = bk_grid(lanes);
  if (kv.val_size == 40)
    hipLaunchKernelGGL(k_block_diff_count<40>, dim3(nb), dim3(BK_TB), 0, st, (const uint8_t *)d_rows, n_rows, (const kv_dev *)kv.d_dev, g, ln,
                       (const uint32_t *)s.run_lo, (const uint32_t *)s.run_hi, s.blk_cnt, s.words, bad);
  else
    hipLaunchKernelGGL(k_block_diff_count<8>, dim3(nb), dim3(BK_TB), 0, st, (const uint8_t *)d_rows, n_rows, (const kv_dev *)kv.d_dev, g, ln,
                       (const uint32_t *)s.run_lo, (const uint32_t *)s.run_hi, s.blk_cnt, s.words, bad);
  sd_launch_scan((const uint32_t *)s.blk_cnt, nb, s.blk_off, s.words + DINT_BLOCK_TOTAL_AT, st);
}
void dint_launch_block_diff_write(const dint_kv &kv, const bk_geom &g, const void *d_ids, uint32_t n_ids, uint64_t lanes, const void *d_rows, uint32_t n_rows,
                                  dint_block_scratch s, void *d_records, uint64_t cap, hipStream_t st) {
  uint32_t *bad = (uint32_t *)(s.words + DINT_BLOCK_BAD_AT);
  const bk_lanes ln = bk_lanes_of(s, d_ids, n_ids);
  const uint32_t nb = bk_grid(lanes);
  if (kv.val_size == 40)
    hipLaunchKernelGGL(k_block_diff_write<40>, dim3(nb), dim3(BK_TB), 0, st, (const uint8_t *)d_rows, n_rows, (const kv_dev *)kv.d_dev, g, ln,
                       (const uint32_t *)s.run_lo, (const uint32_t *)s.run_hi, (const uint64_t *)s.blk_off, (uint8_t *)d_records, cap, bad);
  else
    hipLaunchKernelGGL(k_block_diff_write<8>, dim3(nb), dim3(BK_TB), 0, st, (const uint8_t *)d_rows, n_rows, (const kv_dev *)kv.d_dev, g, ln,
                       (const uint32_t *)s.run_lo, (const uint32_t *)s.run_hi, (const uint64_t *)s.blk_off, (uint8_t *)d_records, cap, bad);
}

static int bk_fail(int rc, const char *what) {
  dint_set_last_error(what);
  return rc;
}

// ---- select: needs no engine ------------------------------------------------------------------------------------------------
extern "C" int64_t dint_state_block_select(const void *d_a, const void *d_b, uint32_t n_blocks, void *d_ids, uint64_t cap, void *stream) {
  if (n_blocks == 0) return 0;
  if (!d_a || !d_b || ((uintptr_t)d_a & 7) || ((uintptr_t)d_b & 7)) return bk_fail(DINT_EINVAL, "block select: two 8-byte aligned digest arrays");
  if ((cap && !d_ids) || ((uintptr_t)d_ids & 3)) return bk_fail(DINT_EINVAL, "block select: cap ids need a 4-byte aligned buffer");
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, d_a) != hipSuccess) {
    (void)hipGetLastError();
    return bk_fail(DINT_EINVAL, "block select: not a device pointer");
  }
  if (hipSetDevice(at.device) != hipSuccess) return bk_fail(DINT_EHIP, "block select: no such device");
  unsigned long long *d_total = nullptr;  // (the call's one word of scratch: allocated and freed by the call, as the view forms do)
  if (hipMalloc((void **)&d_total, sizeof *d_total) != hipSuccess) {
    (void)hipGetLastError();
    return bk_fail(DINT_ENOMEM, "block select: out of device memory");
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_block_select, dim3(1), dim3(1024), 0, st, (const unsigned long long *)d_a, (const unsigned long long *)d_b, n_blocks, (uint32_t *)d_ids,
                     d_ids ? cap : 0, d_total);
  hipError_t err = hipGetLastError();
  unsigned long long total = 0;
  if (err == hipSuccess) err = hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, st);
  const hipError_t serr = hipStreamSynchronize(st);  // (the one synchronisation of the call)
  if (err == hipSuccess) err = serr;
  (void)hipFree(d_total);
  if (err != hipSuccess) {
    char msg[160];
    snprintf(msg, sizeof msg, "block select: %s", hipGetErrorString(err));
    return bk_fail(DINT_EHIP, msg);
  }
  return (int64_t)total;
}

// ---- the host forms (include/dint_driver.h): the same state_block.h / state_sync.h functions over a view in host memory ----------
namespace {
struct bk_host_ld {
  static inline uint32_t u32(const uint8_t *p) { return si_ld32(p); }
  static inline uint64_t u64(const uint8_t *p) { return si_ld64(p); }
};
// the valid rows of one bucket in chain order, as the device's ss_chain reaches them: from `head`, KV_MAX_CHAIN entries at most,
// ending quietly at a link that is neither the inline entry nor inside the pool
struct bk_host_chain {
  std::vector<const uint8_t *> ent;  // per row its entry ...
  std::vector<uint32_t> slot;        // ... and slot
  uint32_t val_size = 0;
  void read(const kv_tab &t, uint64_t b) {
    ent.clear();
    slot.clear();
    val_size = t.val_size;
    uint32_t link = si_ld32(kv_entry_ptr(t, b, KV_INLINE) + offsetof(kv_hdr, head));
    for (uint32_t steps = 0; steps < KV_MAX_CHAIN && (link == KV_INLINE || (link >= 2u && link - 2u < t.pool_cap)); steps++) {
      const uint8_t *e = kv_entry_ptr(t, b, link);
      for (uint32_t s = 0; s < 4; s++)
        if (e[KV_VALID_OFF + s] && ent.size() < SS_WALK_BOUND) {
          ent.push_back(e);
          slot.push_back(s);
        }
      link = si_ld32(e + offsetof(kv_hdr, next));
    }
  }
  uint64_t begin() const { return 0; }
  uint64_t next(uint64_t p) const { return p + 1; }
  bool ok(uint64_t p) const { return p < ent.size(); }
  bool same(uint64_t p, uint64_t q) const { return p == q; }
  uint64_t key(uint64_t p) const { return si_ld64(ent[p] + 8 * slot[p]); }
  uint32_t ver(uint64_t p) const { return si_ld32(ent[p] + 32 + 4 * slot[p]); }
  uint32_t val32(uint64_t p, uint32_t w) const { return si_ld32(ent[p] + KV_VAL_OFF + slot[p] * val_size + 4 * w); }
  uint64_t find(uint64_t k) const {
    for (uint64_t p = 0; p < ent.size(); p++)
      if (key(p) == k) return p;
    return ent.size();
  }
};
struct bk_host_emit {
  uint8_t *out;
  uint64_t at, cap;
  uint32_t table, val_size;
  uint64_t kinds[4];
  template <class L, class P>
  void operator()(uint32_t kind, const L &l, P p) {
    kinds[kind]++;
    if (at < cap) {
      uint32_t w[16];
      ss_fill_record(w, kind, l, p, table, val_size);
      memcpy(out + at * 64, w, 64);
    }
    at++;
  }
};
// view -> tables and geometry; 0 or DINT_EINVAL
int bk_host_open(const dint_tables_view *view, uint64_t B, dint_kv *kv, bk_geom *g) {
  int dummy = 0;
  if (int rc = dint_view_kv(view, &dummy, DINT_KV_MAX_TABLES, kv)) return rc;
  if (!dint_block_geom(*kv, B, g)) return bk_fail(DINT_EINVAL, "block_buckets: a power of two, 64 .. 2^20");
  return 0;
}
bool bk_host_ids_ok(const bk_geom &g, const uint32_t *ids, uint32_t n_ids) {
  for (uint32_t j = 0; j < n_ids; j++)
    if (ids[j] >= bk_blocks(g) || (j > 0 && ids[j - 1] >= ids[j])) return false;
  return true;
}
void bk_fill_stats(dint_block_stats *out, const bk_geom &g, uint64_t total) {
  if (!out) return;
  memset(out, 0, sizeof *out);
  out->total = total;
  out->n_blocks = bk_blocks(g);
  out->n_tables = g.n_tables;
  out->block_buckets = 1u << g.shift;
  for (uint32_t t = 0; t < g.n_tables; t++) out->blocks[t] = g.first[t + 1] - g.first[t];
}
}  // namespace

void dint_block_fill_stats(dint_block_stats *out, const bk_geom &g, uint64_t total) { bk_fill_stats(out, g, total); }

extern "C" int64_t dint_state_block_digest_host(const dint_tables_view *view, uint64_t block_buckets, dint_block_digest *out, uint64_t cap_blocks,
                                                dint_block_stats *out_stats) {
  dint_kv kv;
  bk_geom g;
  if (int rc = bk_host_open(view, block_buckets, &kv, &g)) return rc;
  bk_fill_stats(out_stats, g, bk_blocks(g));
  if (!out) return bk_blocks(g);
  if (cap_blocks < bk_blocks(g)) return bk_fail(DINT_EINVAL, "block digest: room for fewer blocks than there are");
  for (uint32_t id = 0; id < bk_blocks(g); id++) {
    const bk_block blk = bk_locate(g, id);
    const kv_tab &t = kv.h.tab[blk.table];
    ss_digest d = {0, 0, 0};
    for (uint64_t b = blk.first; b < blk.first + blk.count; b++) {
      struct {
        const kv_tab &t;
        uint64_t b;
        bool link_ok(uint32_t link) const { return link - 2u < t.pool_cap; }
        void links(uint32_t link, uint32_t &validw, uint32_t &next) const {
          validw = si_ld32(kv_entry_ptr(t, b, link) + KV_VALID_OFF);
          next = si_ld32(kv_entry_ptr(t, b, link) + offsetof(kv_hdr, next));
        }
      } ch = {t, b};
      (void)si_chain_walk(si_ld32(kv_entry_ptr(t, b, KV_INLINE) + offsetof(kv_hdr, head)), ch, [&](uint32_t, uint32_t link, uint32_t validw) {
        const uint8_t *e = kv_entry_ptr(t, b, link);
        for (uint32_t s = 0; s < 4; s++)
          if ((validw >> (8 * s)) & 0xFFu) {
            const uint8_t *val = e + KV_VAL_OFF + s * t.val_size;
            ss_digest_add(d, ss_row_hash(si_ld64(e + 8 * s), si_ld32(e + 32 + 4 * s), blk.table, t.val_size, [val](uint32_t k) { return si_ld64(val + 8 * k); }));
          }
        return true;
      });
    }
    out[id].rows = d.rows; out[id].sum = d.sum; out[id].xr = d.xr; out[id].reserved = 0;
  }
  return bk_blocks(g);
}

extern "C" int64_t dint_state_block_rows_host(const dint_tables_view *view, uint64_t block_buckets, const uint32_t *ids, uint32_t n_ids, void *records,
                                              uint64_t cap, dint_block_stats *out_stats) {
  dint_kv kv;
  bk_geom g;
  if (int rc = bk_host_open(view, block_buckets, &kv, &g)) return rc;
  if ((n_ids && !ids) || (cap && !records)) return bk_fail(DINT_EINVAL, "null argument");
  if (!bk_host_ids_ok(g, ids, n_ids)) return bk_fail(DINT_EINVAL, bk_bad_name(BK_BAD_IDS));
  try {
    bk_host_chain ch;
    bk_host_emit em = {(uint8_t *)records, 0, cap, 0, kv.val_size, {0, 0, 0, 0}};
    for (uint32_t j = 0; j < n_ids; j++) {
      const bk_block blk = bk_locate(g, ids[j]);
      em.table = blk.table;
      for (uint64_t b = blk.first; b < blk.first + blk.count; b++) {
        ch.read(kv.h.tab[blk.table], b);
        for (uint64_t p = 0; ch.ok(p); p++)
          if (ch.find(ch.key(p)) == p) em(SS_ONLY_A, ch, p);
      }
    }
    bk_fill_stats(out_stats, g, em.at);
    return (int64_t)std::min(em.at, cap);
  } catch (const std::bad_alloc &) {
    return bk_fail(DINT_ENOMEM, "block rows: out of memory");
  }
}

extern "C" int64_t dint_state_block_diff_host(const dint_tables_view *view, uint64_t block_buckets, const uint32_t *ids, uint32_t n_ids, const void *rows,
                                              uint64_t n_rows, void *records, uint64_t cap, dint_diff_stats *out_stats) {
  dint_kv kv;
  bk_geom g;
  if (int rc = bk_host_open(view, block_buckets, &kv, &g)) return rc;
  if ((n_ids && !ids) || (n_rows && !rows) || (cap && !records) || n_rows > BK_MAX_ROWS) return bk_fail(DINT_EINVAL, "null argument, or too many rows");
  if (!bk_host_ids_ok(g, ids, n_ids)) return bk_fail(DINT_EINVAL, bk_bad_name(BK_BAD_IDS));
  const uint8_t *rec = (const uint8_t *)rows;
  auto place = [&](uint64_t i) {
    return bk_row_place<bk_host_ld>(rec + i * 64, g, kv.h.shard_index, kv.h.shard_count,
                                    [&](uint64_t key, uint32_t table) { return dint_hash_key(key) % kv.hash_size[table]; });
  };
  // the check: the whole list before anything is written
  uint32_t bad = 0;
  uint64_t prev = 0, run = 0;
  for (uint64_t i = 0; i < n_rows; i++) {
    const bk_place p = place(i);
    if (p.bad) {
      bad |= p.bad;
      continue;
    }
    if (bk_find_id(ids, n_ids, bk_id_of(g, p.table, p.bucket)) == n_ids) bad |= BK_BAD_HOME;
    if (i > 0 && prev > p.order()) bad |= BK_BAD_ORDER;
    run = i > 0 && prev == p.order() ? run + 1 : 1;
    if (run > BK_MAX_RUN) bad |= BK_BAD_RUN;
    prev = p.order();
  }
  if (bad) return bk_fail(DINT_EINVAL, bk_bad_name(bad));
  try {
    bk_host_chain cb;
    bk_host_emit em = {(uint8_t *)records, 0, cap, 0, kv.val_size, {0, 0, 0, 0}};
    uint64_t at = 0;  // the next row of the list
    for (uint32_t j = 0; j < n_ids; j++) {
      const bk_block blk = bk_locate(g, ids[j]);
      em.table = blk.table;
      for (uint64_t b = blk.first; b < blk.first + blk.count; b++) {
        const uint64_t want = ((uint64_t)blk.table << 56) | b;
        uint64_t end = at;
        while (end < n_rows && place(end).order() == want) end++;
        const bk_run<bk_host_ld> a = {rec + at * 64, (uint32_t)(end - at)};
        cb.read(kv.h.tab[blk.table], b);
        ss_bucket_diff(a, cb, kv.val_size, SS_WALK_BOUND, em);
        at = end;
      }
    }
    if (out_stats) {
      memset(out_stats, 0, sizeof *out_stats);
      out_stats->total = em.at;
      out_stats->only_a = em.kinds[SS_ONLY_A]; out_stats->only_b = em.kinds[SS_ONLY_B];
      out_stats->val_differs = em.kinds[SS_VAL]; out_stats->ver_only = em.kinds[SS_VER];
    }
    return (int64_t)std::min(em.at, cap);
  } catch (const std::bad_alloc &) {
    return bk_fail(DINT_ENOMEM, "block diff: out of memory");
  }
}
