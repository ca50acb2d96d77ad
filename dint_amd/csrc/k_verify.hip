// k_verify.hip -- are an engine's tables and overflow pool structurally sound?  (include/dint_abi.h dint_state_verify, driven by
// engine.hip; the rule lives in state_verify.h, which the host form at the end of this file shares.)  Not on a request's path.
//
//   k_verify_chains   k_state_stats's shape: one lane per bucket, the workgroups striding over the table.  A lane walks its chain
//                     (state_dev.h sd_bucket under state_image.h si_chain_walk) and claims every overflow entry it reaches with
//                     ONE compare-and-swap on the entry's own owner word; the key vector -- the same sector as the links -- is
//                     loaded only of an entry with a valid slot.  Sums in registers, one partial report per workgroup.
//   k_verify_lists    one lane per list, the 192 lists of a table one workgroup, all tables one launch, behind the chains.
//   k_verify_pool     one lane per pool entry, striding: the owner word and 4 bytes of the header.  When a reclaim may follow,
//                     also the unaccounted entries per 256 pool entries.
//   k_verify_sum      one workgroup per table adds up the partials (k_state_digest_sum's shape); longest_list is a maximum.
//   k_verify_compact / k_verify_relink   the reclaim: ranks from state_dev.h k_state_scan and sd_block_excl_scan, the entries
//                     ascending into an array, then every entry's pool_next from the entry 64 ranks ahead.  Both look at the
//                     table's summed report on the device and do nothing when it forbids the reclaim: no host round trip.
// No atomic but the claim; no table content makes a kernel read or write outside the table's buffers or loop without bound.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/dint_abi.h"
#include "../../include/dint_driver.h"
#include "dint_kernels.h"
#include "dint_kv.h"
#include "state_dev.h"
#include "state_image.h"
#include "state_rehash.h"
#include "state_verify.h"

#define SV_TB SD_TB
#define SV_GRID DINT_STATE_VERIFY_GRID
#define SV_PARTS DINT_STATE_VERIFY_PARTS
#define SV_SUM_TB 1024u  // 32 groups of 32 threads, thread w of a group word w

static_assert(SV_WORDS == DINT_STATE_VERIFY_WORDS && sizeof(dint_table_verify) == 8 * SV_WORDS, "a report is a dint_table_verify");
static_assert(offsetof(dint_table_verify, pool_top) == 8 * SV_POOL_TOP && offsetof(dint_table_verify, linked) == 8 * SV_LINKED &&
              offsetof(dint_table_verify, unaccounted) == 8 * SV_UNACCOUNTED && offsetof(dint_table_verify, longest_list) == 8 * SV_LONGEST_LIST &&
              offsetof(dint_table_verify, cross_linked) == 8 * SV_CROSS && offsetof(dint_table_verify, list_bad_links) == 8 * SV_LIST_BAD_LINKS &&
              offsetof(dint_table_verify, stray_rows) == 8 * SV_STRAY_ROWS && offsetof(dint_table_verify, odd_valid_bytes) == 8 * SV_ODD_BYTES &&
              offsetof(dint_table_verify, reclaimed) == 8 * SV_RECLAIMED && offsetof(dint_table_verify, stray_rows_cleared) == 8 * SV_STRAY_CLEARED &&
              offsetof(dint_table_verify, reserved) == 8 * SV_LEAKED_ROWS,
              "the words of state_verify.h are the fields of dint_table_verify");
static_assert(DINT_VERIFY_RECLAIM == DINT_VERIFY_RECLAIM_BIT && DINT_VIEW_CTL_BYTES == SV_CTL_BYTES && DINT_KV_CTL_BYTES == SV_CTL_BYTES,
              "one flag, one control block");

// K per-lane sums to the workgroup's partial report: sum k is word word[k] of part[0 .. SV_WORDS), every other word 0
template <uint32_t K>
__device__ static inline void sv_store_partial(const uint64_t (&s)[K], const uint32_t (&word)[K], unsigned long long *part) {
  __shared__ uint64_t red[SV_TB / 64][K];
  __shared__ uint64_t fin[SV_WORDS];
  const uint32_t tid = threadIdx.x;
  uint64_t ws[K];
#pragma unroll
  for (uint32_t k = 0; k < K; k++) ws[k] = sd_wave_sum_u64(s[k]);
  if ((tid & 63u) == 0) {
#pragma unroll
    for (uint32_t k = 0; k < K; k++) red[tid >> 6][k] = ws[k];
  }
  if (tid < SV_WORDS) fin[tid] = 0;
  __syncthreads();
  if (tid < K) {
    uint64_t v = 0;
    for (uint32_t w = 0; w < blockDim.x / 64; w++) v += red[w][tid];
    uint32_t at = 0;
#pragma unroll
    for (uint32_t k = 0; k < K; k++)
      if (k == tid) at = word[k];
    fin[at] = v;
  }
  __syncthreads();
  if (tid < SV_WORDS) part[tid] = fin[tid];
}

__device__ static inline uint32_t sv_dev_top(const kv_tab &t) {
  return sv_top(*(const volatile KV_G(uint32_t) *)t.pool_top, t.pool_cap);
}

// the accessor of state_verify.h sv_chain_stage over a bucket in HBM
struct sv_dev_chain {
  sd_bucket ch;
  uint32_t *owner;
  dint_mod mod;
  uint32_t shard_index, shard_count;
  __device__ inline uint32_t head() const { return ch.head(); }
  __device__ inline bool link_ok(uint32_t link) const { return ch.link_ok(link); }
  __device__ inline void links(uint32_t link, uint32_t &validw, uint32_t &next) const { ch.links(link, validw, next); }
  __device__ inline void keys(uint32_t link, uint64_t k[4]) const { ch.keys(link, k); }
  __device__ inline uint32_t inline_validw() const { return ch.lv.x; }
  __device__ inline uint32_t claim(uint32_t p, uint32_t code) const { return atomicCAS(owner + p, 0u, code); }  // (p < pool_cap: link_ok)
  __device__ inline uint64_t home(uint64_t key) const {
    return sr_local_bucket(dint_fastmod(dint_hash_key(key), mod), shard_index, shard_count);
  }
};

// part[SV_WORDS * workgroup ..] = what the buckets this workgroup walked add (state_verify.h words)
__global__ void __launch_bounds__(SV_TB) k_verify_chains(kv_tab t, dint_mod mod, uint32_t shard_index, uint32_t shard_count,
                                                         uint32_t *__restrict__ owner, unsigned long long *__restrict__ part) {
  const uint32_t tid = threadIdx.x, top = sv_dev_top(t);
  uint64_t s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (uint64_t base = (uint64_t)blockIdx.x * SV_TB; base < t.n_local; base += (uint64_t)gridDim.x * SV_TB) {
    const uint64_t b = base + tid;
    if (b < t.n_local) {
      const sv_dev_chain a = {sd_bucket_at(t, b), owner, mod, shard_index, shard_count};
      const sv_chain r = sv_chain_stage(a, b, top);
      s[0] += r.rows; s[1] += r.linked; s[2] += r.cross; s[3] += r.beyond; s[4] += r.bad;
      s[5] += r.stray_entries; s[6] += r.stray_rows; s[7] += r.misplaced; s[8] += r.odd;
    }
  }
  const uint32_t word[9] = {SV_ROWS, SV_LINKED, SV_CROSS, SV_BEYOND_TOP, SV_BAD_CHAINS, SV_STRAY_ENTRIES, SV_STRAY_ROWS, SV_MISPLACED, SV_ODD_BYTES};
  sv_store_partial(s, word, part + (size_t)SV_WORDS * blockIdx.x);
}

// the lists of every table: workgroup = table, lane = list
struct sv_dev_list {
  const kv_tab &t;
  uint32_t *owner;
  __device__ inline uint32_t pool_next(uint32_t p) const { return *(const volatile KV_G(uint32_t) *)(t.pool_next + p); }
  __device__ inline uint32_t claim(uint32_t p, uint32_t code) const { return atomicCAS(owner + p, 0u, code); }  // (p < pool_cap: the rule)
};
struct sv_list_args {
  kv_tab tab[DINT_KV_MAX_TABLES];
  uint32_t *owner[DINT_KV_MAX_TABLES];
  unsigned long long *part[DINT_KV_MAX_TABLES];  // the table's one partial of this stage
};
__global__ void __launch_bounds__(SV_LISTS) k_verify_lists(sv_list_args a) {
  __shared__ uint32_t longest[SV_LISTS / 64];
  const uint32_t tid = threadIdx.x, table = blockIdx.x;
  const kv_tab &t = a.tab[table];
  const uint32_t top = sv_dev_top(t);
  const unsigned long long *hw = tid < KV_NLISTS ? t.free_head + tid : t.pend_head + (tid - KV_NLISTS);
  const uint32_t head_link = (uint32_t)*(const volatile KV_G(unsigned long long) *)hw;
  const sv_dev_list l = {t, a.owner[table]};
  const sv_list r = sv_list_stage(l, tid, head_link, t.pool_cap, top);
  const bool fr = sv_list_is_free(tid);
  const uint32_t wl = sd_wave_max_u32(r.claimed);
  if ((tid & 63u) == 0) longest[tid >> 6] = wl;
  const uint64_t s[5] = {fr ? r.claimed : 0u, fr ? 0u : r.claimed, r.cross, r.beyond, r.bad_links};
  const uint32_t word[5] = {SV_FREE, SV_PENDING, SV_CROSS, SV_BEYOND_TOP, SV_LIST_BAD_LINKS};
  sv_store_partial(s, word, a.part[table]);  // (its barriers order `longest` as well)
  if (tid == SV_LONGEST_LIST) {  // (the thread that stored the word's 0 just now)
    uint32_t m = 0;
    for (uint32_t w = 0; w < SV_LISTS / 64; w++) m = max(m, longest[w]);
    a.part[table][SV_LONGEST_LIST] = m;
  }
}

// blk_cnt (may be null): [block of 256 pool entries] the unaccounted entries among them
__global__ void __launch_bounds__(SV_TB) k_verify_pool(kv_tab t, const uint32_t *__restrict__ owner, uint32_t *__restrict__ blk_cnt,
                                                       unsigned long long *__restrict__ part) {
  __shared__ uint32_t red[SV_TB / 64][1];
  const uint32_t tid = threadIdx.x, top = sv_dev_top(t);
  uint64_t s[4] = {0, 0, 0, 0};
  for (uint64_t base = (uint64_t)blockIdx.x * SV_TB; base < t.pool_cap; base += (uint64_t)gridDim.x * SV_TB) {  // (uniform in the workgroup)
    const uint64_t p = base + tid;
    sv_pool r = {0, 0, 0, 0};
    if (p < t.pool_cap) {
      const uint32_t validw = *(const KV_G(uint32_t) *)(kv_entry_ptr(t, 0, (uint32_t)p + 2u) + KV_VALID_OFF);
      r = sv_pool_entry((uint32_t)p, owner[p], validw, top);
      s[0] += r.unaccounted; s[1] += r.stray_entries; s[2] += r.stray_rows; s[3] += r.leaked_rows;
    }
    if (blk_cnt) {
      const uint32_t v[1] = {r.unaccounted};
      __syncthreads();  // (the previous round's readers of red are done)
      sd_block_sum(red, v);
      if (tid == 0) blk_cnt[base / SV_TB] = sd_block_total(red, 0);
    }
  }
  const uint32_t word[4] = {SV_UNACCOUNTED, SV_STRAY_ENTRIES, SV_STRAY_ROWS, SV_LEAKED_ROWS};
  sv_store_partial(s, word, part + (size_t)SV_WORDS * blockIdx.x);
}

// out[SV_WORDS t ..] = the n[t] partials of table t (workgroup = table) at part + SV_WORDS * SV_PARTS * t combined
struct sv_sum_args {
  uint32_t n[DINT_KV_MAX_TABLES];
  uint32_t pool_cap[DINT_KV_MAX_TABLES];
  const uint32_t *pool_top[DINT_KV_MAX_TABLES];
};
__global__ void __launch_bounds__(SV_SUM_TB) k_verify_sum(const unsigned long long *__restrict__ part, sv_sum_args a,
                                                          unsigned long long *__restrict__ out) {
  constexpr uint32_t G = SV_SUM_TB / SV_WORDS;
  __shared__ uint64_t red[G][SV_WORDS];
  const uint32_t tid = threadIdx.x, table = blockIdx.x, w = tid & (SV_WORDS - 1u), g = tid / SV_WORDS;
  const unsigned long long *p = part + (size_t)SV_WORDS * SV_PARTS * table;
  const uint32_t n = a.n[table];
  const bool is_max = w == SV_LONGEST_LIST;
  uint64_t v = 0;
  for (uint32_t k = g; k < n; k += G) {
    const uint64_t x = p[(size_t)SV_WORDS * k + w];
    v = is_max ? (v > x ? v : x) : v + x;
  }
  red[g][w] = v;
  __syncthreads();
  if (tid < SV_WORDS) {
    for (uint32_t k = 1; k < G; k++) {
      const uint64_t x = red[k][tid];
      v = is_max ? (v > x ? v : x) : v + x;
    }
    if (tid == SV_POOL_CAP) v = a.pool_cap[table];
    if (tid == SV_POOL_TOP) v = *(const volatile KV_G(uint32_t) *)a.pool_top[table];  // (raw: a failed insert may have left it above the pool's size)
    out[(size_t)SV_WORDS * table + tid] = v;
  }
}

// ---- reclaim -------------------------------------------------------------------------------------------------------------------
// may the call reclaim?  Only when no table's summed report forbids it: a refused call writes not a byte
__device__ static inline bool sv_dev_reclaim_ok(const unsigned long long *all, uint32_t n_tables) {
  bool ok = true;
  for (uint32_t t = 0; t < n_tables; t++) ok = ok && sv_reclaim_ok((const uint64_t *)all + (size_t)SV_WORDS * t);
  return ok;
}
// all = every table's summed report, w = this table's.  Workgroup = 256 pool entries: leaked[rank] = every unaccounted entry, ascending; heads[] = the
// free lists' head words as they are now
__global__ void __launch_bounds__(SV_TB) k_verify_compact(kv_tab t, const uint32_t *__restrict__ owner, const unsigned long long *__restrict__ all,
                                                          uint32_t n_tables, uint32_t table, const uint64_t *__restrict__ blk_off, uint32_t *__restrict__ leaked,
                                                          unsigned long long *__restrict__ heads) {
  __shared__ uint32_t red[SV_TB / 64];
  const unsigned long long *w = all + (size_t)SV_WORDS * table;
  if (!sv_dev_reclaim_ok(all, n_tables) || w[SV_UNACCOUNTED] == 0) return;  // (the whole workgroup)
  const uint32_t tid = threadIdx.x, top = sv_dev_top(t);
  const uint64_t p = (uint64_t)blockIdx.x * SV_TB + tid;
  const uint32_t flag = p < top && owner[p] == 0;  // (top <= pool_cap)
  const uint64_t r = blk_off[blockIdx.x] + sd_block_excl_scan(red, flag);
  if (flag && r < t.pool_cap) leaked[r] = (uint32_t)p;
  if (blockIdx.x == 0 && tid < KV_NLISTS) heads[tid] = *(const volatile KV_G(unsigned long long) *)(t.free_head + tid);
}
// thread = rank r of the n unaccounted entries
__global__ void __launch_bounds__(SV_TB) k_verify_relink(kv_tab t, const unsigned long long *__restrict__ all, uint32_t n_tables, uint32_t table,
                                                         const uint32_t *__restrict__ leaked, const unsigned long long *__restrict__ heads) {
  const unsigned long long *w = all + (size_t)SV_WORDS * table;
  if (!sv_dev_reclaim_ok(all, n_tables)) return;
  const uint64_t n = w[SV_UNACCOUNTED] < t.pool_cap ? w[SV_UNACCOUNTED] : t.pool_cap, r = (uint64_t)blockIdx.x * SV_TB + threadIdx.x;
  if (r >= n) return;
  const uint32_t p = leaked[r];
  if (p >= t.pool_cap) return;  // (never: the compaction wrote entries below the pool's top)
  const uint32_t ahead = r + KV_NLISTS < n ? leaked[r + KV_NLISTS] : 0u;
  const uint64_t old = heads[r & (KV_NLISTS - 1u)];
  t.pool_next[p] = sv_reclaim_next(r, n, ahead, old);
  const sd_v2 zero = {0u, 0u};
  *(KV_G(sd_v2) *)(kv_entry_ptr(t, 0, p + 2u) + KV_VALID_OFF) = zero;  // {validw, next}
  if (r < KV_NLISTS) t.free_head[r] = sv_reclaim_head(old, p);
}

// ------------------------------------------------------------------------------------------------------ host side
static uint64_t sv_owner_words(const dint_kv &kv) {
  uint64_t n = 0;
  for (uint32_t t = 0; t < kv.n_tables; t++) n += kv.h.tab[t].pool_cap;
  return n;
}
static uint64_t sv_blocks(const dint_kv &kv) {
  uint64_t n = 0;
  for (uint32_t t = 0; t < kv.n_tables; t++) n += ((uint64_t)kv.h.tab[t].pool_cap + SV_TB - 1) / SV_TB;
  return n;
}
void dint_verify_free(dint_verify_scratch &s) {
  hipFree(s.owner); hipFree(s.part); hipFree(s.out); hipFree(s.leaked); hipFree(s.blk_cnt); hipFree(s.blk_off); hipFree(s.heads);
  s = dint_verify_scratch{};
}
int dint_verify_alloc(const dint_kv &kv, dint_verify_scratch &s, uint32_t flags) {
  for (uint32_t t = 0; t < kv.n_tables; t++)
    if (kv.h.tab[t].n_local >= SV_MAX_LOCAL) {
      dint_set_last_error("a table of 2^32 - 256 local buckets or more");
      return DINT_EINVAL;
    }
  const uint64_t owner_n = sv_owner_words(kv), blk_n = sv_blocks(kv);
  bool ok = true;
  if (!s.part) {
    ok = hipMalloc((void **)&s.owner, (owner_n ? owner_n : 1) * sizeof(uint32_t)) == hipSuccess &&
         hipMalloc((void **)&s.part, (size_t)DINT_KV_MAX_TABLES * SV_PARTS * SV_WORDS * sizeof(unsigned long long)) == hipSuccess &&
         hipMalloc((void **)&s.out, ((size_t)DINT_KV_MAX_TABLES * SV_WORDS + 1) * sizeof(unsigned long long)) == hipSuccess;
    s.owner_n = owner_n;
  }
  if (ok && (flags & DINT_VERIFY_RECLAIM) && !s.heads) {
    ok = hipMalloc((void **)&s.leaked, (owner_n ? owner_n : 1) * sizeof(uint32_t)) == hipSuccess &&
         hipMalloc((void **)&s.blk_cnt, (blk_n ? blk_n : 1) * sizeof(uint32_t)) == hipSuccess &&
         hipMalloc((void **)&s.blk_off, (blk_n ? blk_n : 1) * sizeof(uint64_t)) == hipSuccess &&
         hipMalloc((void **)&s.heads, (size_t)DINT_KV_MAX_TABLES * KV_NLISTS * sizeof(unsigned long long)) == hipSuccess;
    s.blk_n = blk_n;
  }
  if (!ok) {
    (void)hipGetLastError();
    dint_verify_free(s);
    dint_set_last_error("table verify: out of device memory for the owner words");
    return DINT_ENOMEM;
  }
  return 0;
}

static uint32_t sv_grid(uint64_t n) {
  const uint64_t nb = (n + SV_TB - 1) / SV_TB;
  return (uint32_t)(nb < 1 ? 1 : nb > SV_GRID ? SV_GRID : nb);
}

void dint_launch_state_verify(const dint_kv &kv, dint_verify_scratch s, uint32_t flags, hipStream_t st, hipEvent_t *ev) {
  const bool reclaim = (flags & DINT_VERIFY_RECLAIM) != 0;
  (void)hipMemsetAsync(s.owner, 0, (s.owner_n ? s.owner_n : 1) * sizeof(uint32_t), st);  // (the call's stream, not the null stream)
  sv_sum_args sa;
  sv_list_args la;
  memset(&sa, 0, sizeof sa);
  memset(&la, 0, sizeof la);
  uint32_t n_chain[DINT_KV_MAX_TABLES];
  uint64_t owner_at = 0;
  if (ev) (void)hipEventRecord(ev[0], st);
  for (uint32_t t = 0; t < kv.n_tables; t++) {
    const kv_tab &tb = kv.h.tab[t];
    unsigned long long *part = s.part + (size_t)SV_WORDS * SV_PARTS * t;
    n_chain[t] = sv_grid(tb.n_local);
    la.tab[t] = tb;
    la.owner[t] = s.owner + owner_at;
    la.part[t] = part + (size_t)SV_WORDS * n_chain[t];
    hipLaunchKernelGGL(k_verify_chains, dim3(n_chain[t]), dim3(SV_TB), 0, st, tb, kv.h.mod[t], kv.h.shard_index, kv.h.shard_count,
                       s.owner + owner_at, part);
    owner_at += tb.pool_cap;
  }
  if (ev) (void)hipEventRecord(ev[1], st);
  hipLaunchKernelGGL(k_verify_lists, dim3(kv.n_tables), dim3(SV_LISTS), 0, st, la);  // (behind every table's chains: one stream)
  if (ev) (void)hipEventRecord(ev[2], st);
  owner_at = 0;
  uint64_t blk_at = 0;
  for (uint32_t t = 0; t < kv.n_tables; t++) {
    const kv_tab &tb = kv.h.tab[t];
    const uint32_t n_pool = sv_grid(tb.pool_cap);
    sa.n[t] = n_chain[t] + 1u + n_pool;
    sa.pool_cap[t] = tb.pool_cap;
    sa.pool_top[t] = tb.pool_top;
    hipLaunchKernelGGL(k_verify_pool, dim3(n_pool), dim3(SV_TB), 0, st, tb, (const uint32_t *)(s.owner + owner_at),
                       reclaim ? s.blk_cnt + blk_at : (uint32_t *)nullptr, s.part + (size_t)SV_WORDS * (SV_PARTS * t + n_chain[t] + 1u));
    owner_at += tb.pool_cap;
    blk_at += ((uint64_t)tb.pool_cap + SV_TB - 1) / SV_TB;
  }
  hipLaunchKernelGGL(k_verify_sum, dim3(kv.n_tables), dim3(SV_SUM_TB), 0, st, (const unsigned long long *)s.part, sa, s.out);
  if (ev) (void)hipEventRecord(ev[3], st);
  if (!reclaim) return;
  owner_at = blk_at = 0;
  for (uint32_t t = 0; t < kv.n_tables; t++) {
    const kv_tab &tb = kv.h.tab[t];
    const uint32_t nb = (uint32_t)(((uint64_t)tb.pool_cap + SV_TB - 1) / SV_TB);
    if (nb) {
      unsigned long long *heads = s.heads + (size_t)KV_NLISTS * t;
      sd_launch_scan<uint32_t>(s.blk_cnt + blk_at, nb, s.blk_off + blk_at, s.out + (size_t)SV_WORDS * DINT_KV_MAX_TABLES, st);
      hipLaunchKernelGGL(k_verify_compact, dim3(nb), dim3(SV_TB), 0, st, tb, (const uint32_t *)(s.owner + owner_at),
                         (const unsigned long long *)s.out, kv.n_tables, t, (const uint64_t *)(s.blk_off + blk_at), s.leaked + owner_at, heads);
      hipLaunchKernelGGL(k_verify_relink, dim3(nb), dim3(SV_TB), 0, st, tb, (const unsigned long long *)s.out, kv.n_tables, t,
                         (const uint32_t *)(s.leaked + owner_at),
                         (const unsigned long long *)heads);
    }
    owner_at += tb.pool_cap;
    blk_at += nb;
  }
}

// the words of every table as the caller sees them; returns DINT_ESTATE when a reclaim was asked for and a table forbids it
static int sv_finish(uint64_t (*h)[SV_WORDS], uint32_t n_tables, uint32_t flags, dint_table_verify *out, uint64_t *reclaimed) {
  int rc = 0;
  uint64_t got = 0;
  char msg[200];
  const bool want = (flags & DINT_VERIFY_RECLAIM) != 0;
  bool all_ok = true;
  for (uint32_t t = 0; t < n_tables; t++) all_ok = all_ok && sv_reclaim_ok(h[t]);
  for (uint32_t t = 0; t < n_tables; t++) {
    const bool ok = sv_reclaim_ok(h[t]);
    if (want && !ok && !rc) {
      snprintf(msg, sizeof msg, "table %u: %llu bad chains, %llu cross-linked entries, %llu entries linked beyond the pool's top, %llu bad list links: nothing reclaimed",
               t, (unsigned long long)h[t][SV_BAD_CHAINS], (unsigned long long)h[t][SV_CROSS], (unsigned long long)h[t][SV_BEYOND_TOP],
               (unsigned long long)h[t][SV_LIST_BAD_LINKS]);
      dint_set_last_error(msg);
      rc = DINT_ESTATE;
    }
    sv_report_finish(h[t], want && all_ok);
    got += h[t][SV_RECLAIMED];
  }
  memcpy(out, h, (size_t)n_tables * sizeof(dint_table_verify));
  if (reclaimed) *reclaimed = got;
  return rc;
}

int dint_verify_collect(const dint_kv &kv, dint_verify_scratch s, uint32_t flags, hipStream_t st, dint_table_verify *out, uint64_t *reclaimed) {
  uint64_t h[DINT_KV_MAX_TABLES][SV_WORDS];
  hipError_t err = hipMemcpyAsync(h, s.out, sizeof h, hipMemcpyDeviceToHost, st);  // (the one synchronisation of the call)
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) {
    char msg[160];
    snprintf(msg, sizeof msg, "table verify: %s", hipGetErrorString(err));
    dint_set_last_error(msg);
    return DINT_EHIP;
  }
  return sv_finish(h, kv.n_tables, flags, out, reclaimed);
}

// ---- the forms over caller-provided memory (include/dint_driver.h) -----------------------------------------------------------
static bool sv_shape(uint32_t workload, uint32_t *n_tables, uint32_t *stride, uint32_t *val_size) {
  switch (workload) {
    case DINT_WL_STORE: *n_tables = 1; *stride = 256; *val_size = 40; return true;
    case DINT_WL_TATP: *n_tables = 5; *stride = 256; *val_size = 40; return true;
    case DINT_WL_SMALLBANK: *n_tables = 2; *stride = 128; *val_size = 8; return true;
    default: return false;
  }
}
static int sv_view_bad(const char *what, uint32_t t) {
  char msg[160];
  snprintf(msg, sizeof msg, "table view: table %u: %s", t, what);
  dint_set_last_error(msg);
  return DINT_EINVAL;
}
// the view's own consistency; then kv = the tables as the launchers and the host form take them (no device memory of its own)
int dint_view_kv(const dint_tables_view *v, const void *out, uint32_t cap_tables, dint_kv *kv) {
  if (!v || !out) {
    dint_set_last_error("null argument");
    return DINT_EINVAL;
  }
  uint32_t n_tables, stride, val_size;
  if (!sv_shape(v->workload, &n_tables, &stride, &val_size)) return sv_view_bad("not a kv workload", 0);
  if (v->n_tables != n_tables) return sv_view_bad("the workload has another number of tables", 0);
  if (v->shard_count == 0 || v->shard_count > 255 || v->shard_index >= v->shard_count) return sv_view_bad("shard_index < shard_count <= 255", 0);
  if (cap_tables < n_tables) {
    char msg[80];
    snprintf(msg, sizeof msg, "%u tables, room for %u", n_tables, cap_tables);
    dint_set_last_error(msg);
    return DINT_EINVAL;
  }
  *kv = dint_kv();
  kv->workload = v->workload;
  kv->n_tables = kv->h.n_tables = n_tables;
  kv->val_size = val_size;
  kv->h.shard_index = v->shard_index;
  kv->h.shard_count = v->shard_count;
  for (uint32_t t = 0; t < n_tables; t++) {
    const dint_table_view &tv = v->table[t];
    if (tv.stride != stride || tv.val_size != val_size) return sv_view_bad("stride or value size is not the workload's", t);
    if (tv.hash_size == 0 || tv.n_local != (tv.hash_size + v->shard_count - 1) / v->shard_count) return sv_view_bad("n_local is not ceil(hash_size / shard_count)", t);
    if (tv.n_local >= SV_MAX_LOCAL || tv.pool_cap > 0xFFFFFFF0u) return sv_view_bad("too many buckets or pool entries", t);
    if (!tv.entries || !tv.ctl || (tv.pool_cap && !tv.pool_next)) return sv_view_bad("a null pointer", t);
    if (((uintptr_t)tv.entries & 15) || ((uintptr_t)tv.ctl & 7) || ((uintptr_t)tv.pool_next & 3)) return sv_view_bad("a pointer that is not aligned", t);
    kv_tab &tb = kv->h.tab[t];
    tb.entries = (uint8_t *)tv.entries;
    tb.n_local = tv.n_local;
    tb.pool_cap = tv.pool_cap;
    tb.stride = stride;
    tb.val_size = val_size;
    tb.pool_top = (uint32_t *)((uint8_t *)tv.ctl + SV_CTL_TOP);
    tb.pool_next = tv.pool_next;
    tb.free_head = (unsigned long long *)((uint8_t *)tv.ctl + SV_CTL_HEADS);
    tb.pend_head = tb.free_head + KV_NLISTS;
    kv->hash_size[t] = tv.hash_size;
    kv->h.mod[t] = dint_make_mod(tv.hash_size);
    kv->entry_bytes[t] = (size_t)(tb.n_local + tb.pool_cap) * stride;
  }
  return 0;
}

extern "C" int dint_state_verify_view(int32_t device, const dint_tables_view *view, dint_table_verify *out, uint32_t cap_tables,
                                      uint32_t flags, void *stream) {
  dint_kv kv;
  if (int rc = dint_view_kv(view, out, cap_tables, &kv)) return rc;
  if (hipSetDevice(device) != hipSuccess) {
    dint_set_last_error("table view: no such device");
    return DINT_EHIP;
  }
  dint_verify_scratch s{};
  if (int rc = dint_verify_alloc(kv, s, flags)) return rc;
  hipStream_t st = (hipStream_t)stream;
  dint_launch_state_verify(kv, s, flags, st);
  int rc = 0;
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    char msg[160];
    snprintf(msg, sizeof msg, "kernel launch: %s", hipGetErrorString(err));
    dint_set_last_error(msg);
    (void)hipStreamSynchronize(st);
    rc = DINT_EHIP;
  } else {
    rc = dint_verify_collect(kv, s, flags, st, out, nullptr);
  }
  dint_verify_free(s);
  return rc ? rc : (int)kv.n_tables;
}

// the accessors of state_verify.h over host memory (the words at any alignment the view's check let through)
struct sv_host_chain {
  const kv_tab &t;
  uint64_t b;
  uint32_t *owner;
  uint64_t hash_size;
  uint32_t shard_index, shard_count;
  const uint8_t *e(uint32_t link) const { return kv_entry_ptr(t, b, link); }
  uint32_t head() const { return si_ld32(e(KV_INLINE) + offsetof(kv_hdr, head)); }
  bool link_ok(uint32_t link) const { return link - 2u < t.pool_cap; }
  void links(uint32_t link, uint32_t &validw, uint32_t &next) const {
    validw = si_ld32(e(link) + KV_VALID_OFF);
    next = si_ld32(e(link) + offsetof(kv_hdr, next));
  }
  void keys(uint32_t link, uint64_t k[4]) const {
    for (uint32_t i = 0; i < 4; i++) k[i] = si_ld64(e(link) + 8 * i);
  }
  uint32_t inline_validw() const { return si_ld32(e(KV_INLINE) + KV_VALID_OFF); }
  uint32_t claim(uint32_t p, uint32_t code) const {
    const uint32_t was = owner[p];
    if (was == 0) owner[p] = code;
    return was;
  }
  uint64_t home(uint64_t key) const { return sr_local_bucket(dint_hash_key(key) % hash_size, shard_index, shard_count); }
};
struct sv_host_list {
  const kv_tab &t;
  uint32_t *owner;
  uint32_t pool_next(uint32_t p) const { return t.pool_next[p]; }
  uint32_t claim(uint32_t p, uint32_t code) const {
    const uint32_t was = owner[p];
    if (was == 0) owner[p] = code;
    return was;
  }
};

extern "C" int dint_state_verify_view_host(const dint_tables_view *view, dint_table_verify *out, uint32_t cap_tables, uint32_t flags) {
  dint_kv kv;
  if (int rc = dint_view_kv(view, out, cap_tables, &kv)) return rc;
  uint64_t h[DINT_KV_MAX_TABLES][SV_WORDS];
  memset(h, 0, sizeof h);
  std::vector<uint32_t> leaked[DINT_KV_MAX_TABLES];
  bool all_ok = true;
  for (uint32_t ti = 0; ti < kv.n_tables; ti++) {
    const kv_tab &t = kv.h.tab[ti];
    uint64_t *w = h[ti];
    const uint32_t raw_top = *t.pool_top, top = sv_top(raw_top, t.pool_cap);
    std::vector<uint32_t> owner((size_t)t.pool_cap + 1, 0u);
    for (uint64_t b = 0; b < t.n_local; b++) {
      const sv_host_chain a = {t, b, owner.data(), kv.hash_size[ti], kv.h.shard_index, kv.h.shard_count};
      sv_report_add_chain(w, sv_chain_stage(a, b, top));
    }
    const sv_host_list l = {t, owner.data()};
    for (uint32_t list = 0; list < SV_LISTS; list++) {
      const unsigned long long hw = list < KV_NLISTS ? t.free_head[list] : t.pend_head[list - KV_NLISTS];
      sv_report_add_list(w, list, sv_list_stage(l, list, (uint32_t)hw, t.pool_cap, top));
    }
    for (uint32_t p = 0; p < t.pool_cap; p++) {
      const sv_pool r = sv_pool_entry(p, owner[p], si_ld32(kv_entry_ptr(t, 0, p + 2u) + KV_VALID_OFF), top);
      sv_report_add_pool(w, r);
      if (r.unaccounted) leaked[ti].push_back(p);
    }
    w[SV_POOL_CAP] = t.pool_cap;
    w[SV_POOL_TOP] = raw_top;
    all_ok = all_ok && sv_reclaim_ok(w);
  }
  for (uint32_t ti = 0; ti < kv.n_tables && (flags & DINT_VERIFY_RECLAIM) && all_ok; ti++) {  // (a refused call writes not a byte)
    const kv_tab &t = kv.h.tab[ti];
    const std::vector<uint32_t> &u = leaked[ti];
    const uint64_t n = u.size();
    unsigned long long old[KV_NLISTS];
    memcpy(old, t.free_head, sizeof old);
    for (uint64_t r = 0; r < n; r++) {
      const uint32_t p = u[r];
      t.pool_next[p] = sv_reclaim_next(r, n, r + KV_NLISTS < n ? u[r + KV_NLISTS] : 0u, old[r & (KV_NLISTS - 1u)]);
      memset(kv_entry_ptr(t, 0, p + 2u) + KV_VALID_OFF, 0, 8);  // {validw, next}
      if (r < KV_NLISTS) t.free_head[r] = sv_reclaim_head(old[r], p);
    }
  }
  const int rc = sv_finish(h, kv.n_tables, flags, out, nullptr);
  return rc ? rc : (int)kv.n_tables;
}
