// k_rehash.hip -- the rows of a set of engines placed into a blank engine of another bucket count without leaving the GPU
// (include/dint_abi.h dint_state_rehash, driven by engine.hip; the layout rule lives in state_rehash.h, which the host form
// at the end of this file shares).  Table by table:
//
//   k_rehash_count    one lane per SOURCE bucket: the valid slots of its chain and the lock words it holds.  Reads the 16-byte
//                     link vector of the inline header; a chain is walked only where that vector says there is one, by
//                     state_image.h si_chain_walk over state_dev.h sd_bucket.  Per workgroup one {rows, locks}
//   k_state_scan      (state_dev.h) exclusive scan of the workgroups' rows of one table -- the sources' workgroups laid end to end in `srcs`
//                     order, so a workgroup's offset is its first row's place in SOURCE ORDER -- and the two totals
//   k_rehash_keys     (the host has read the totals by now)  the count again, a scan inside the workgroup; every valid slot,
//                     in chain order, becomes a 32-bit sort key -- the destination's local bucket, or n_local for a row that is
//                     home to another shard -- and a 64-bit locator {source, entry, slot}
//   radix sort        (key, locator) pairs, stable, over the sr_key_bits(n_local) bits in use: stability carries source order
//   k_rehash_heads    position p of the sorted rows: p where a run of equal keys starts, else 0; an inclusive max-scan makes
//                     that every row's run head, so r = p - head is the row's number in its destination bucket
//   k_rehash_flags    {this row opens an entry, ... an overflow entry} packed into one 64-bit word per row; the rows placed,
//                     the longest chain, a bucket that needs more than SI_MAX_RUN overflow entries (one atomic per wave and
//                     word: the plan is the slowest stage and this is the likely reason -- DESIGN.md 8d names the way out).  The exclusive sum-scan
//                     of the words numbers the entries (high half) and IS the pool index of every overflow entry (low half);
//                     its total is the table's need.  (the host reads the totals of all tables once, and refuses here)
//   k_rehash_list     the sorted position of the first row of every destination entry, by entry number
//   k_rehash_build    one lane group per destination entry (16 lanes per 256-byte entry, 8 per 128-byte entry): the group
//                     gathers its <= 4 rows through their locators -- a lane loads what its own 16-byte vector holds, all of
//                     it before its one store -- and writes the entry whole: keys, versions, valid bytes, next, head, values;
//                     lock bytes, counters and owner keys zero.  No atomics and no read of the destination: every entry has
//                     one lane group.  One workgroup's first lane sets pool_top.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <new>
#include <numeric>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "../../include/dint_abi.h"
#include "../../include/dint_driver.h"
#include "dint_kernels.h"
#include "dint_kv.h"
#include "state_dev.h"
#include "state_image.h"
#include "state_rehash.h"

#define RH_TB SD_TB  // threads per workgroup, every kernel here

// ------------------------------------------------------------------------------------------------------ the sources
// the valid slots of the chain of bucket ch; false = the chain does not end within KV_MAX_CHAIN entries, visits its inline entry
// twice or leaves the pool: nothing is read through such a link
__device__ static inline bool rh_rows(const sd_bucket &ch, uint32_t &rows) {
  return si_chain_walk(ch.head(), ch, [&](uint32_t, uint32_t, uint32_t validw) {
    rows += si_valid_count(validw);
    return true;
  });
}

// lock_mode: state_image.h SI_LOCKS_*
// blk[workgroup] = {valid slots, lock words held} of its 256 buckets; *badw |= 1: a chain that cannot be walked
__global__ void __launch_bounds__(RH_TB) k_rehash_count(kv_tab t, uint32_t lock_mode, sd_v2 *__restrict__ blk, uint32_t *badw) {
  __shared__ uint32_t red[RH_TB / 64][2];
  const uint64_t b = (uint64_t)blockIdx.x * RH_TB + threadIdx.x;
  uint32_t rows = 0, locks = 0;
  if (b < t.n_local) {
    const sd_bucket ch = sd_bucket_at(t, b);
    if (!rh_rows(ch, rows)) atomicOr(badw, 1u);
    locks = ch.locks_held(lock_mode);
  }
  sd_block_sum(red, {rows, locks});
  if (threadIdx.x == 0) blk[blockIdx.x] = sd_v2{sd_block_total(red, 0), sd_block_total(red, 1)};
}

// where the rows of one source go: the destination's bucket count, shard and local buckets
struct rh_dst {
  dint_mod size, count;  // % hash_size, / shard_count
  uint32_t index;
  uint64_t n_local;
};
// the destination's local bucket of `key`, or d.n_local: home to another shard
__device__ static inline uint32_t rh_key(uint64_t key, const rh_dst &d) {
  const uint64_t g = dint_fastmod(dint_hash_key(key), d.size);
  uint64_t local = g;
  if (d.count.d > 1) {
    const uint64_t q = sd_div(g, d.count);
    local = g - q * d.count.d == d.index ? q : SR_FOREIGN;
  }
  return local < d.n_local ? (uint32_t)local : (uint32_t)d.n_local;
}

// key[at] / loc[at] of every valid slot of source `src`, at = the slot's place in source order (n = the table's rows over all
// sources as the count pass found them: nothing is stored beyond, whatever the tables say by now)
__global__ void __launch_bounds__(RH_TB) k_rehash_keys(kv_tab t, uint32_t src, const uint64_t *__restrict__ blk_off, rh_dst d,
                                                       uint32_t *__restrict__ key, uint64_t *__restrict__ loc, uint64_t n) {
  __shared__ uint32_t red[RH_TB / 64];
  const uint64_t b = (uint64_t)blockIdx.x * RH_TB + threadIdx.x;
  uint32_t rows = 0;
  if (b < t.n_local && !rh_rows(sd_bucket_at(t, b), rows)) rows = 0;  // (the count pass has refused such a source already)
  const uint32_t before = sd_block_excl_scan(red, rows);
  if (!rows) return;
  uint64_t at = blk_off[blockIdx.x] + before;
  const sd_bucket ch = sd_bucket_at(t, b);
  si_chain_walk(ch.head(), ch, [&](uint32_t, uint32_t link, uint32_t validw) {
    if (!validw) return true;
    const uint64_t e = link == KV_INLINE ? b : t.n_local + (link - 2u);
    const KV_G(uint64_t) *k = (const KV_G(uint64_t) *)(t.entries + e * t.stride);
#pragma unroll
    for (uint32_t i = 0; i < 4; i++)
      if ((validw >> (8 * i)) & 0xFFu) {
        if (at < n) {
          key[at] = rh_key(k[i], d);
          loc[at] = sr_loc(src, e, i);
        }
        at++;
      }
    return true;
  });
}

// ------------------------------------------------------------------------------------------------------ the plan
// head[p] = p where a run of equal keys starts, else 0 (an inclusive max-scan then gives every row its run's first position)
__global__ void __launch_bounds__(RH_TB) k_rehash_heads(const uint32_t *__restrict__ key, uint32_t n, uint32_t *__restrict__ head) {
  const uint32_t p = blockIdx.x * RH_TB + threadIdx.x;
  if (p >= n) return;
  head[p] = (p > 0 && key[p - 1] != key[p]) ? p : 0u;
}

// f[p] = {opens an entry : high half, opens an overflow entry : low half} of sorted row p, f[n] = 0 (the exclusive scan's
// total lands there); w[0] += rows placed, w[1] = max(entries of a bucket); *badw |= 2: a bucket beyond SI_MAX_RUN
__global__ void __launch_bounds__(RH_TB) k_rehash_flags(const uint32_t *__restrict__ key, const uint32_t *__restrict__ head, uint32_t n,
                                                        uint32_t n_local, unsigned long long *__restrict__ f, unsigned long long *w,
                                                        uint32_t *badw) {
  const uint32_t p = blockIdx.x * RH_TB + threadIdx.x;
  uint32_t live = 0, entries = 0;
  if (p < n) {
    const uint32_t k = key[p], r = p - head[p];
    live = k < n_local;
    f[p] = live ? ((unsigned long long)sr_opens_entry(r) << 32 | (unsigned long long)sr_opens_overflow(r)) : 0ull;
    if (live && (p + 1 == n || key[p + 1] != k)) entries = sr_entries(r + 1u);  // (the bucket's last row)
  } else if (p == n) {
    f[p] = 0ull;
  }
  live = sd_wave_sum_u32(live);
  entries = sd_wave_max_u32(entries);
  if ((threadIdx.x & 63) == 0) {
    if (live) atomicAdd(w, (unsigned long long)live);
    if (entries) atomicMax(w + 1, (unsigned long long)entries);
    if (entries > SI_MAX_RUN + 1u) atomicOr(badw, 2u);
  }
}

// elist[x] = the sorted position of the first row of destination entry x (x = the high half of the scan at that row)
__global__ void __launch_bounds__(RH_TB) k_rehash_list(const uint32_t *__restrict__ key, const uint32_t *__restrict__ head,
                                                       const unsigned long long *__restrict__ scan, uint32_t n, uint32_t n_local,
                                                       uint32_t *__restrict__ elist) {
  const uint32_t p = blockIdx.x * RH_TB + threadIdx.x;
  if (p >= n || key[p] >= n_local || !sr_opens_entry(p - head[p])) return;
  const uint32_t x = (uint32_t)(scan[p] >> 32);
  if (x < n) elist[x] = p;
}

// ------------------------------------------------------------------------------------------------------ the build
// the source entry a locator names
__device__ static inline const uint8_t *rh_src(const uint8_t *const *__restrict__ src_entries, uint64_t loc, uint32_t stride) {
  return src_entries[sr_loc_src(loc)] + sr_loc_entry(loc) * stride;
}

// n_ent destination entries, entry x built from the sorted rows elist[x] .. (at most four of one key[]); need = the table's
// overflow entries (pool_top afterwards: the destination was blank)
template <uint32_t STRIDE>
__global__ void __launch_bounds__(RH_TB) k_rehash_build(kv_tab t, const uint32_t *__restrict__ key, const uint64_t *__restrict__ loc,
                                                        const unsigned long long *__restrict__ scan, const uint32_t *__restrict__ elist,
                                                        uint32_t n, uint32_t n_ent, uint32_t need,
                                                        const uint8_t *const *__restrict__ src_entries) {
  constexpr uint32_t VPE = STRIDE / 16, EPS = RH_TB / VPE, VAL = STRIDE == 256 ? 40u : 8u;
  const uint32_t v = threadIdx.x % VPE;
  const uint64_t x = (uint64_t)blockIdx.x * EPS + threadIdx.x / VPE;
  if (blockIdx.x == 0 && threadIdx.x == 0) KV_ST(uint32_t, t.pool_top, need);
  if (x >= n_ent) return;
  const uint32_t p = elist[x];
  if (p >= n) return;
  const uint32_t b = key[p];
  uint32_t m = 1;  // rows of this entry: p .. p + m - 1
  while (m < 4 && p + m < n && key[p + m] == b) m++;
  const bool is_inline = p == 0 || key[p - 1] != b;
  const uint32_t pool = (uint32_t)scan[p];  // (an overflow entry: its pool index)
  if (b >= t.n_local || (!is_inline && pool >= t.pool_cap)) return;  // (the host has compared the need with the pool: never taken)
  const uint64_t at = is_inline ? (uint64_t)b : t.n_local + pool;
  sd_v4 o = {0, 0, 0, 0};
  if (v < 2) {  // keys of rows 2 v, 2 v + 1
#pragma unroll
    for (uint32_t h = 0; h < 2; h++) {
      const uint32_t row = 2 * v + h;
      if (row < m) {
        const uint64_t l = loc[p + row];
        const uint64_t k = *((const KV_G(uint64_t) *)rh_src(src_entries, l, STRIDE) + sr_loc_slot(l));
        o[2 * h] = (uint32_t)k;
        o[2 * h + 1] = (uint32_t)(k >> 32);
      }
    }
  } else if (v == 2) {  // versions
#pragma unroll
    for (uint32_t row = 0; row < 4; row++)
      if (row < m) {
        const uint64_t l = loc[p + row];
        o[row] = *((const KV_G(uint32_t) *)(rh_src(src_entries, l, STRIDE) + offsetof(kv_hdr, ver)) + sr_loc_slot(l));
      }
  } else if (v == SI_LINK_VEC) {  // {validw, next, head, lockw = 0}
    const bool more = p + 4 < n && key[p + 4] == b;
    o.x = sr_validw(m);
    o.y = more ? sr_link(1, (uint32_t)scan[p + 4]) : KV_NULL;
    o.z = is_inline ? KV_INLINE : KV_NULL;
  } else {  // values, 8 bytes at a time: byte off of the entry's value area belongs to row off / VAL
#pragma unroll
    for (uint32_t h = 0; h < 2; h++) {
      const uint32_t off = 16 * (v - 4) + 8 * h, row = off / VAL;
      if (off < 4 * VAL && row < m) {
        const uint64_t l = loc[p + row];
        const uint64_t w = *(const KV_G(uint64_t) *)(rh_src(src_entries, l, STRIDE) + KV_VAL_OFF + sr_loc_slot(l) * VAL + off % VAL);
        o[2 * h] = (uint32_t)w;
        o[2 * h + 1] = (uint32_t)(w >> 32);
      }
    }
  }
  *((KV_G(sd_v4) *)(t.entries + at * STRIDE) + v) = o;
}

// ------------------------------------------------------------------------------------------------------ host side
static inline uint32_t rh_blocks(uint64_t n) { return (uint32_t)((n + RH_TB - 1) / RH_TB); }

uint32_t dint_rehash_blocks(const dint_kv *const *srcs, uint32_t n_srcs) {
  uint64_t nb = 0;
  for (uint32_t t = 0; t < srcs[0]->n_tables; t++)
    for (uint32_t s = 0; s < n_srcs; s++) nb += rh_blocks(srcs[s]->h.tab[t].n_local);
  return (uint32_t)std::min<uint64_t>(nb, 0xFFFFFFFFull);
}

void dint_launch_rehash_count(const dint_kv *const *srcs, uint32_t n_srcs, dint_rehash_scratch s, hipStream_t st) {
  (void)hipMemsetAsync(s.words, 0, DINT_REHASH_WORDS * sizeof(unsigned long long), st);
  const uint32_t lock_mode = si_lock_mode(srcs[0]->workload);
  uint32_t at = 0;
  for (uint32_t t = 0; t < srcs[0]->n_tables; t++) {
    const uint32_t at0 = at;
    for (uint32_t k = 0; k < n_srcs; k++) {
      const kv_tab &tb = srcs[k]->h.tab[t];
      const uint32_t nb = rh_blocks(tb.n_local);
      hipLaunchKernelGGL(k_rehash_count, dim3(nb), dim3(RH_TB), 0, st, tb, lock_mode, (sd_v2 *)s.blk + at,
                         (uint32_t *)(s.words + DINT_REHASH_BAD_AT));
      at += nb;
    }
    sd_launch_scan((const sd_v2 *)s.blk + at0, at - at0, s.blk_off + at0, s.words + DINT_REHASH_TABLE_WORDS * t, st);
  }
}

// temporary storage of the sort and the two scans of a table of n rows (the largest of the three), or -1
int64_t dint_rehash_tmp_bytes(uint64_t n, uint64_t dst_n_local, hipStream_t st) {
  size_t a = 0, b = 0, c = 0;
  if (rocprim::radix_sort_pairs(nullptr, a, (const uint32_t *)nullptr, (uint32_t *)nullptr, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                (size_t)n, 0u, sr_key_bits(dst_n_local), st) != hipSuccess)
    return -1;
  if (rocprim::inclusive_scan(nullptr, b, (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n, rocprim::maximum<uint32_t>(), st) != hipSuccess)
    return -1;
  if (rocprim::exclusive_scan(nullptr, c, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, 0ull, (size_t)n + 1,
                              rocprim::plus<unsigned long long>(), st) != hipSuccess)
    return -1;
  return (int64_t)std::max(a, std::max(b, c));
}

// table t: keys, sort, plan.  n = its rows over all sources (1 .. SR_MAX_ROWS), row_at = where its rows start in the arrays
// that are kept for the build.  ev (or nullptr): four events recorded before the keys, the sort, the plan and after it.
bool dint_launch_rehash_plan(uint32_t t, const dint_kv *const *srcs, uint32_t n_srcs, uint32_t blk_at, const dint_kv &dst, uint64_t n,
                             uint64_t row_at, dint_rehash_scratch s, hipStream_t st, hipEvent_t *ev) {
  const kv_tab &dt = dst.h.tab[t];
  const rh_dst d = {dst.h.mod[t], dint_make_mod(dst.h.shard_count), dst.h.shard_index, dt.n_local};
  uint32_t *key = s.key_out + row_at, *elist = s.elist + row_at;
  uint64_t *loc = s.loc_out + row_at;
  unsigned long long *scan = s.scan + row_at + t;  // (n + 1 words per table)
  unsigned long long *w = s.words + DINT_REHASH_TABLE_WORDS * t;
  const uint32_t n32 = (uint32_t)n, nl = (uint32_t)dt.n_local;
  if (ev) (void)hipEventRecord(ev[0], st);
  uint32_t at = blk_at;
  for (uint32_t k = 0; k < n_srcs; k++) {
    const kv_tab &tb = srcs[k]->h.tab[t];
    const uint32_t nb = rh_blocks(tb.n_local);
    hipLaunchKernelGGL(k_rehash_keys, dim3(nb), dim3(RH_TB), 0, st, tb, k, (const uint64_t *)s.blk_off + at, d, s.key_in, s.loc_in, n);
    at += nb;
  }
  if (ev) (void)hipEventRecord(ev[1], st);
  size_t bytes = s.tmp_bytes;
  if (rocprim::radix_sort_pairs(s.tmp, bytes, (const uint32_t *)s.key_in, key, (const uint64_t *)s.loc_in, loc, (size_t)n, 0u,
                                sr_key_bits(dt.n_local), st) != hipSuccess)
    return false;
  if (ev) (void)hipEventRecord(ev[2], st);
  hipLaunchKernelGGL(k_rehash_heads, dim3(rh_blocks(n)), dim3(RH_TB), 0, st, (const uint32_t *)key, n32, s.head);
  bytes = s.tmp_bytes;
  if (rocprim::inclusive_scan(s.tmp, bytes, (const uint32_t *)s.head, s.head, (size_t)n, rocprim::maximum<uint32_t>(), st) != hipSuccess) return false;
  hipLaunchKernelGGL(k_rehash_flags, dim3(rh_blocks(n + 1)), dim3(RH_TB), 0, st, (const uint32_t *)key, (const uint32_t *)s.head, n32, nl, scan,
                     w + 3, (uint32_t *)(s.words + DINT_REHASH_BAD_AT));
  bytes = s.tmp_bytes;
  if (rocprim::exclusive_scan(s.tmp, bytes, (const unsigned long long *)scan, scan, 0ull, (size_t)n + 1, rocprim::plus<unsigned long long>(), st) !=
      hipSuccess)
    return false;
  (void)hipMemcpyAsync(w + 2, scan + n, sizeof(unsigned long long), hipMemcpyDeviceToDevice, st);
  hipLaunchKernelGGL(k_rehash_list, dim3(rh_blocks(n)), dim3(RH_TB), 0, st, (const uint32_t *)key, (const uint32_t *)s.head,
                     (const unsigned long long *)scan, n32, nl, elist);
  if (ev) (void)hipEventRecord(ev[3], st);
  return true;
}

// table t: its n_ent entries from the plan's arrays; need = its overflow entries
void dint_launch_rehash_build(uint32_t t, const dint_kv &dst, uint64_t n, uint64_t row_at, uint64_t n_ent, uint32_t need,
                              const uint8_t *const *d_src_entries, dint_rehash_scratch s, hipStream_t st) {
  if (!n_ent) return;
  const kv_tab &dt = dst.h.tab[t];
  const uint32_t *key = s.key_out + row_at, *elist = s.elist + row_at;
  const uint64_t *loc = s.loc_out + row_at;
  const unsigned long long *scan = s.scan + row_at + t;
  const uint32_t per = RH_TB / (dt.stride / 16), nb = (uint32_t)((n_ent + per - 1) / per);
  if (dt.stride == 256)
    hipLaunchKernelGGL(k_rehash_build<256>, dim3(nb), dim3(RH_TB), 0, st, dt, key, loc, scan, elist, (uint32_t)n, (uint32_t)n_ent, need, d_src_entries);
  else
    hipLaunchKernelGGL(k_rehash_build<128>, dim3(nb), dim3(RH_TB), 0, st, dt, key, loc, scan, elist, (uint32_t)n, (uint32_t)n_ent, need, d_src_entries);
}

// ---- the host form (include/dint_driver.h): the same state_rehash.h rule over keys in source order -------------------------
extern "C" int64_t dint_state_rehash_place_host(const uint64_t *keys, uint64_t n, uint64_t hash_size, uint32_t shard_index,
                                                uint32_t shard_count, uint64_t *bucket_out, uint32_t *link_out, uint32_t *slot_out) {
  if (shard_count == 0) shard_count = 1;
  if (hash_size == 0 || shard_index >= shard_count || n > SR_MAX_ROWS || (n && (!keys || !bucket_out || !link_out || !slot_out))) return DINT_EINVAL;
  try {
    std::vector<uint32_t> idx(n);
    std::iota(idx.begin(), idx.end(), 0u);
    for (uint64_t i = 0; i < n; i++) bucket_out[i] = sr_local_bucket(dint_hash_key(keys[i]) % hash_size, shard_index, shard_count);
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return bucket_out[x] < bucket_out[y]; });  // (foreign rows last)
    uint64_t pool = 0;  // the running scan of "opens an overflow entry"
    uint32_t r = 0, link = KV_NULL;
    for (uint64_t p = 0; p < n; p++) {
      const uint32_t i = idx[p];
      if (bucket_out[i] == SR_FOREIGN) { link_out[i] = KV_NULL; slot_out[i] = 0; continue; }
      r = (p > 0 && bucket_out[idx[p - 1]] == bucket_out[i]) ? r + 1 : 0;
      if (sr_opens_entry(r)) {
        if (sr_opens_overflow(r) && pool >= 0xFFFFFFF0ull) return DINT_ENOMEM;
        link = sr_link(sr_chain_pos(r), (uint32_t)pool);
        if (sr_opens_overflow(r)) pool++;
      }
      link_out[i] = link;
      slot_out[i] = sr_slot(r);
    }
    return (int64_t)pool;
  } catch (const std::bad_alloc &) {
    return DINT_ENOMEM;
  }
}
