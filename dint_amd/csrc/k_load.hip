// k_load.hip -- rows loaded into a server's tables, and the reference's population generated, without leaving the GPU
// (include/dint_abi.h dint_load_rows_device / dint_populate_device, driven by engine.hip; the rule lives in state_load.h, which
// the host forms at the end of this file share).
//
// DIRECT LOAD of n rows in insertion order into a table that has taken nothing since creation / reset:
//   k_load_keys     one lane per row: a 32-bit sort key -- the local bucket, or n_local for a row home to another shard -- and
//                   the row number; the foreign rows counted (one atomic per workgroup that has any)
//   radix sort      (key, row number) pairs, stable, over sr_key_bits(n_local) bits: stability carries insertion order
//   k_load_heads    position p where a run of equal keys starts, else 0; an inclusive max-scan makes that every row's run head,
//                   so r = p - head is the row's number in its bucket
//   k_load_flags    {opens an entry, opens an overflow entry} in one 64-bit word per row; a bucket's last row leaves the bucket's
//                   row count at its run head; the longest chain and a chain beyond KV_MAX_CHAIN by an atomic that only a wave
//                   which would raise the word pays (the rows placed are n less the foreign rows).  The exclusive sum-scan
//                   numbers the entries (high half) and IS every overflow entry's pool index (low half); its total is the
//                   table's need.  (the host reads the words once, and refuses here)
//   k_load_list     the sorted position of the first row of every destination entry, by entry number
//   k_load_build    one lane group per destination entry (16 lanes per 256-byte entry, 8 per 128-byte entry): keys, versions, the
//                   {validw, next} pair -- next = the entry opened BEFORE this one, head = the bucket's last: newest entry first --
//                   and the values, 16 bytes per lane; lock bytes, owner keys and counters are not stored.  No atomic decides a
//                   position, nothing of the destination is read.  One workgroup's first lane stores pool_top.
// PASS PATH (the table holds something): k_load_msgs forms DINT_KV_LOAD_OP messages from the device arrays, one wave lane per
// message byte, into the engine's request slot; the load-mode passes are engine.hip's.
// GENERATION: k_load_gen, one workgroup per tile of SL_TILE subscribers, one lane per subscriber.  A group with a constant draw
// count jumps to its state (sl_lcg_jump) and its row offset is a product; for the two data-dependent groups the tile's first
// state and row offset come from the tile table (ld_tiles, a host pre-pass cached per process), lane 0 walks the tile's draw
// rule into LDS, and then every lane writes its subscriber's rows: rows leave in insertion order as SoA.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "../../include/dint_abi.h"
#include "../../include/dint_driver.h"
#include "dint_kernels.h"
#include "dint_kv.h"
#include "state_dev.h"
#include "state_load.h"

#define LD_TB SD_TB

static_assert(SL_WL_STORE == DINT_WL_STORE && SL_WL_TATP == DINT_WL_TATP && SL_WL_SMALLBANK == DINT_WL_SMALLBANK, "state_load.h restates the workloads");
static_assert(SL_TILE == LD_TB, "one lane per subscriber of a tile");

// ------------------------------------------------------------------------------------------------------ the plan
struct ld_dst {
  dint_mod size, count;  // % hash_size, / shard_count
  uint32_t index;
  uint64_t n_local;
};
// key[i] = the local bucket of keys[i] or n_local (foreign), idx[i] = i (either may be null: the count alone); *foreign += the foreign rows
__global__ void __launch_bounds__(LD_TB) k_load_keys(const uint64_t *__restrict__ keys, uint32_t n, ld_dst d, uint32_t *__restrict__ key,
                                                     uint32_t *__restrict__ idx, unsigned long long *foreign) {
  const uint32_t i = blockIdx.x * LD_TB + threadIdx.x;
  uint32_t f = 0;
  if (i < n) {
    const uint64_t g = dint_fastmod(dint_hash_key(keys[i]), d.size);
    uint64_t local = g;
    if (d.count.d > 1) {
      const uint64_t q = sd_div(g, d.count);
      local = g - q * d.count.d == d.index ? q : SR_FOREIGN;
    }
    const uint32_t k = local < d.n_local ? (uint32_t)local : (uint32_t)d.n_local;
    f = k == (uint32_t)d.n_local;
    if (key) {
      key[i] = k;
      idx[i] = i;
    }
  }
  __shared__ uint32_t red[LD_TB / 64][1];
  sd_block_sum(red, {f});
  if (threadIdx.x == 0)
    if (const uint32_t tot = sd_block_total(red, 0)) atomicAdd(foreign, (unsigned long long)tot);
}

__global__ void __launch_bounds__(LD_TB) k_load_heads(const uint32_t *__restrict__ key, uint32_t n, uint32_t *__restrict__ head) {
  const uint32_t p = blockIdx.x * LD_TB + threadIdx.x;
  if (p >= n) return;
  head[p] = (p > 0 && key[p - 1] != key[p]) ? p : 0u;
}

// f[p] = {opens an entry : high half, opens an overflow entry : low half} of sorted row p, f[n] = 0 (the exclusive scan's total
// lands there); cnt[run head] = the bucket's rows; *w = max(entries of a bucket); *badw |= 2: a chain too long
__global__ void __launch_bounds__(LD_TB) k_load_flags(const uint32_t *__restrict__ key, const uint32_t *__restrict__ head, uint32_t n, uint32_t n_local,
                                                      unsigned long long *__restrict__ f, uint32_t *__restrict__ cnt, unsigned long long *w,
                                                      uint32_t *badw) {
  const uint32_t p = blockIdx.x * LD_TB + threadIdx.x;
  uint32_t entries = 0;
  if (p < n) {
    const uint32_t k = key[p], h = head[p], r = p - h;
    const bool live = k < n_local;
    f[p] = live ? ((unsigned long long)sr_opens_entry(r) << 32 | (unsigned long long)sr_opens_overflow(r)) : 0ull;
    if (live && (p + 1 == n || key[p + 1] != k)) {  // (the bucket's last row)
      entries = sr_entries(r + 1u);
      cnt[h] = r + 1u;
    }
  } else if (p == n) {
    f[p] = 0ull;
  }
  entries = sd_wave_max_u32(entries);
  // (nearly every wave ends a bucket: the word is read first, and only a wave that would raise it pays the atomic)
  if ((threadIdx.x & 63) == 0 && entries > *(volatile unsigned long long *)w) {
    atomicMax(w, (unsigned long long)entries);
    if (sl_chain_too_long(entries)) atomicOr(badw, 2u);
  }
}

__global__ void __launch_bounds__(LD_TB) k_load_list(const uint32_t *__restrict__ key, const uint32_t *__restrict__ head,
                                                     const unsigned long long *__restrict__ scan, uint32_t n, uint32_t n_local,
                                                     uint32_t *__restrict__ elist) {
  const uint32_t p = blockIdx.x * LD_TB + threadIdx.x;
  if (p >= n || key[p] >= n_local || !sr_opens_entry(p - head[p])) return;
  const uint32_t x = (uint32_t)(scan[p] >> 32);
  if (x < n) elist[x] = p;
}

// ------------------------------------------------------------------------------------------------------ the build
// n_ent destination entries, entry x built from the sorted rows elist[x] .. (at most four of one bucket); need = the table's
// overflow entries (pool_top afterwards: the table held nothing)
template <uint32_t STRIDE>
__global__ void __launch_bounds__(LD_TB) k_load_build(kv_tab t, const uint32_t *__restrict__ key, const uint32_t *__restrict__ idx,
                                                      const uint32_t *__restrict__ head, const uint32_t *__restrict__ cnt,
                                                      const unsigned long long *__restrict__ scan, const uint32_t *__restrict__ elist, uint32_t n,
                                                      uint32_t n_ent, uint32_t need, const uint64_t *__restrict__ keys,
                                                      const uint32_t *__restrict__ vers, const uint8_t *__restrict__ vals) {
  constexpr uint32_t VPE = STRIDE / 16, EPS = LD_TB / VPE, VAL = STRIDE == 256 ? 40u : 8u;
  const uint32_t v = threadIdx.x % VPE;
  const uint64_t x = (uint64_t)blockIdx.x * EPS + threadIdx.x / VPE;
  if (blockIdx.x == 0 && threadIdx.x == 0) KV_ST(uint32_t, t.pool_top, need);
  if (x >= n_ent) return;
  const uint32_t p = elist[x];
  if (p >= n) return;
  const uint32_t b = key[p], h = head[p];
  if (b >= t.n_local || h > p) return;
  const uint32_t k = cnt[h], r0 = p - h, c = sr_chain_pos(r0);  // the bucket's rows, this entry's first row and chain position
  if (r0 >= k || (uint64_t)h + k > n) return;
  const uint32_t m = min(4u, k - r0);
  const uint32_t pool = (uint32_t)scan[p];  // (an overflow entry: its pool index)
  if (c > 0 && pool >= t.pool_cap) return;  // (the host has compared the need with the pool: never taken)
  uint8_t *e = t.entries + (c == 0 ? (uint64_t)b : t.n_local + pool) * STRIDE;
  sd_v4 o = {0, 0, 0, 0};
  if (v < 2) {  // keys of rows 2 v, 2 v + 1
#pragma unroll
    for (uint32_t j = 0; j < 2; j++) {
      const uint32_t row = 2 * v + j;
      if (row < m) {
        const uint64_t kk = keys[idx[p + row]];
        o[2 * j] = (uint32_t)kk;
        o[2 * j + 1] = (uint32_t)(kk >> 32);
      }
    }
  } else if (v == 2) {  // versions
#pragma unroll
    for (uint32_t row = 0; row < 4; row++)
      if (row < m && vers) o[row] = vers[idx[p + row]];
  } else if (v == SI_LINK_VEC) {  // {validw, next}, and in the inline entry head: lockw is left as it is
    const sd_v2 l = {sr_validw(m), sl_next(c, c >= 2 ? (uint32_t)scan[p - 4] : 0u)};
    *(KV_G(sd_v2) *)(e + KV_VALID_OFF) = l;
    if (c == 0) {
      const uint32_t last = sr_entries(k) - 1u;  // the newest entry
      KV_ST(uint32_t, e + offsetof(kv_hdr, head), sr_link(last, last ? (uint32_t)scan[h + 4u * last] : 0u));
    }
    return;
  } else {  // values, 8 bytes at a time: byte off of the entry's value area belongs to row off / VAL
    if (16 * (v - 4) >= 4 * VAL) return;  // (counters, owner keys: not stored)
#pragma unroll
    for (uint32_t j = 0; j < 2; j++) {
      const uint32_t off = 16 * (v - 4) + 8 * j, row = off / VAL;
      if (off < 4 * VAL && row < m) {
        const uint64_t w = *(const uint64_t *)(vals + (uint64_t)idx[p + row] * VAL + off % VAL);
        o[2 * j] = (uint32_t)w;
        o[2 * j + 1] = (uint32_t)(w >> 32);
      }
    }
  }
  *((KV_G(sd_v4) *)e + v) = o;
}

// ------------------------------------------------------------------------------------------------------ the pass path
// message j of the pass = row first + j as a DINT_KV_LOAD_OP request: lane l of the wave stores byte l
__global__ void __launch_bounds__(LD_TB) k_load_msgs(dint_kv_fmt f, uint32_t table, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vers,
                                                     const uint8_t *__restrict__ vals, uint64_t first, uint32_t m, uint8_t *__restrict__ req) {
  const uint32_t j = blockIdx.x * (LD_TB / 64) + threadIdx.x / 64, l = threadIdx.x & 63;
  if (j >= m || l >= f.msg) return;
  const uint64_t i = first + j;
  uint32_t byte = 0;
  if (l == f.type) byte = DINT_KV_LOAD_OP;
  else if (l == f.table) byte = table;
  else if (l - f.key < 8u) byte = (uint32_t)(keys[i] >> (8u * (l - f.key)));
  else if (l - f.val < f.val_size) byte = vals[i * f.val_size + (l - f.val)];
  else if (l - f.ver < 4u) byte = vers ? vers[i] >> (8u * (l - f.ver)) : 0u;
  req[(uint64_t)j * f.msg + l] = (uint8_t)byte;
}

// ------------------------------------------------------------------------------------------------------ generation
template <uint32_t VW>
struct ld_write_emit {
  uint64_t *keys, *vals;
  uint64_t at, cap;
  uint32_t which;
  __device__ inline void operator()(uint32_t w_, uint64_t key, const uint64_t *w) {
    if (w_ != which) return;
    if (at < cap) {
      keys[at] = key;
#pragma unroll
      for (uint32_t j = 0; j < VW; j++) vals[at * VW + j] = w[j];
    }
    at++;
  }
};
// table `which` of `group` for subscribers 0 .. n_subs - 1: keys[] / vals[][VW words] in insertion order, nothing stored at or
// beyond row cap.  tile_state / tile_rows: the tile table of a data-dependent group (tile_rows: of table `which`), else unused
template <uint32_t VW>
__global__ void __launch_bounds__(LD_TB) k_load_gen(uint32_t group, uint32_t which, uint64_t n_subs, const uint64_t *__restrict__ tile_state,
                                                    const uint64_t *__restrict__ tile_rows, uint64_t *__restrict__ keys, uint64_t *__restrict__ vals,
                                                    uint64_t cap) {
  __shared__ uint64_t st[SL_TILE];
  __shared__ uint32_t ro[SL_TILE];
  const uint64_t s0 = (uint64_t)blockIdx.x * SL_TILE, s = s0 + threadIdx.x;
  const uint32_t draws = sl_draws(group);
  uint64_t g, at;
  if (draws == SL_DRAWS_VAR) {
    if (threadIdx.x == 0) {  // the draw rule alone over the tile: every subscriber's first state and row offset
      uint64_t gg = tile_state[blockIdx.x];
      uint32_t run = 0;
      for (uint32_t i = 0; i < SL_TILE && s0 + i < n_subs; i++) {
        st[i] = gg;
        ro[i] = run;
        uint32_t r[2];
        sl_skip_sub(group, s0 + i, gg, r);
        run += r[which & 1u];
      }
    }
    __syncthreads();
    if (s >= n_subs) return;
    g = st[threadIdx.x];
    at = tile_rows[blockIdx.x] + ro[threadIdx.x];
  } else {
    if (s >= n_subs) return;
    g = sl_lcg_jump(SL_SEED, (uint64_t)draws * s);
    at = s * sl_rows_fixed(group);
  }
  ld_write_emit<VW> em{keys, vals, at, cap, which};
  sl_gen_sub(group, s, g, em);
}

// ------------------------------------------------------------------------------------------------------ host side
static inline uint32_t ld_blocks(uint64_t n, uint32_t per = LD_TB) { return (uint32_t)((n + per - 1) / per); }
static inline ld_dst ld_dst_of(const dint_kv &kv, uint32_t t) {
  return ld_dst{kv.h.mod[t], dint_make_mod(kv.h.shard_count), kv.h.shard_index, kv.h.tab[t].n_local};
}

// temporary storage of the sort and the two scans of n rows (the largest of the three), or -1
int64_t dint_load_tmp_bytes(uint64_t n, uint64_t n_local, hipStream_t st) {
  size_t a = 0, b = 0, c = 0;
  if (rocprim::radix_sort_pairs(nullptr, a, (const uint32_t *)nullptr, (uint32_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n, 0u,
                                sr_key_bits(n_local), st) != hipSuccess)
    return -1;
  if (rocprim::inclusive_scan(nullptr, b, (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n, rocprim::maximum<uint32_t>(), st) != hipSuccess)
    return -1;
  if (rocprim::exclusive_scan(nullptr, c, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, 0ull, (size_t)n + 1,
                              rocprim::plus<unsigned long long>(), st) != hipSuccess)
    return -1;
  return (int64_t)std::max(a, std::max(b, c));
}

// the foreign rows of keys[0 .. n) into s.words[DINT_LOAD_FOREIGN_AT] (s.words cleared first)
void dint_launch_load_count(const dint_kv &kv, uint32_t t, const uint64_t *d_keys, uint64_t n, dint_load_scratch s, hipStream_t st) {
  (void)hipMemsetAsync(s.words, 0, DINT_LOAD_WORDS * sizeof(unsigned long long), st);
  if (n)
    hipLaunchKernelGGL(k_load_keys, dim3(ld_blocks(n)), dim3(LD_TB), 0, st, d_keys, (uint32_t)n, ld_dst_of(kv, t), (uint32_t *)nullptr, (uint32_t *)nullptr,
                       s.words + DINT_LOAD_FOREIGN_AT);
}

// keys, sort, plan of n rows (1 .. SL_MAX_ROWS) for table t; the result words into s.words.  ev (or nullptr): four events
// recorded before the keys, the sort, the plan and after it.  false = a sort or scan failed
bool dint_launch_load_plan(const dint_kv &kv, uint32_t t, const uint64_t *d_keys, uint64_t n, dint_load_scratch s, hipStream_t st, hipEvent_t *ev) {
  const kv_tab &tb = kv.h.tab[t];
  const uint32_t n32 = (uint32_t)n, nl = (uint32_t)tb.n_local;
  uint32_t *head = s.key_a, *cnt = s.idx_a;  // (the unsorted arrays are free once the sort has run)
  (void)hipMemsetAsync(s.words, 0, DINT_LOAD_WORDS * sizeof(unsigned long long), st);
  if (ev) (void)hipEventRecord(ev[0], st);
  hipLaunchKernelGGL(k_load_keys, dim3(ld_blocks(n)), dim3(LD_TB), 0, st, d_keys, n32, ld_dst_of(kv, t), s.key_a, s.idx_a, s.words + DINT_LOAD_FOREIGN_AT);
  if (ev) (void)hipEventRecord(ev[1], st);
  size_t bytes = s.tmp_bytes;
  if (rocprim::radix_sort_pairs(s.tmp, bytes, (const uint32_t *)s.key_a, s.key_b, (const uint32_t *)s.idx_a, s.idx_b, (size_t)n, 0u,
                                sr_key_bits(tb.n_local), st) != hipSuccess)
    return false;
  if (ev) (void)hipEventRecord(ev[2], st);
  hipLaunchKernelGGL(k_load_heads, dim3(ld_blocks(n)), dim3(LD_TB), 0, st, (const uint32_t *)s.key_b, n32, head);
  bytes = s.tmp_bytes;
  if (rocprim::inclusive_scan(s.tmp, bytes, (const uint32_t *)head, head, (size_t)n, rocprim::maximum<uint32_t>(), st) != hipSuccess) return false;
  hipLaunchKernelGGL(k_load_flags, dim3(ld_blocks(n + 1)), dim3(LD_TB), 0, st, (const uint32_t *)s.key_b, (const uint32_t *)head, n32, nl, s.scan, cnt,
                     s.words + DINT_LOAD_LONGEST_AT, (uint32_t *)(s.words + DINT_LOAD_BAD_AT));
  bytes = s.tmp_bytes;
  if (rocprim::exclusive_scan(s.tmp, bytes, (const unsigned long long *)s.scan, s.scan, 0ull, (size_t)n + 1, rocprim::plus<unsigned long long>(), st) !=
      hipSuccess)
    return false;
  (void)hipMemcpyAsync(s.words + DINT_LOAD_TOTAL_AT, s.scan + n, sizeof(unsigned long long), hipMemcpyDeviceToDevice, st);
  hipLaunchKernelGGL(k_load_list, dim3(ld_blocks(n)), dim3(LD_TB), 0, st, (const uint32_t *)s.key_b, (const uint32_t *)head,
                     (const unsigned long long *)s.scan, n32, nl, s.elist);
  if (ev) (void)hipEventRecord(ev[3], st);
  return true;
}

// table t's n_ent entries from the plan's arrays and the caller's rows; need = its overflow entries
void dint_launch_load_build(const dint_kv &kv, uint32_t t, const uint64_t *d_keys, const uint32_t *d_vers, const void *d_vals, uint64_t n, uint64_t n_ent,
                            uint32_t need, dint_load_scratch s, hipStream_t st) {
  if (!n_ent) return;
  const kv_tab &tb = kv.h.tab[t];
  const uint32_t per = LD_TB / (tb.stride / 16), nb = ld_blocks(n_ent, per);
  if (tb.stride == 256)
    hipLaunchKernelGGL(k_load_build<256>, dim3(nb), dim3(LD_TB), 0, st, tb, (const uint32_t *)s.key_b, (const uint32_t *)s.idx_b, (const uint32_t *)s.key_a,
                       (const uint32_t *)s.idx_a, (const unsigned long long *)s.scan, (const uint32_t *)s.elist, (uint32_t)n, (uint32_t)n_ent, need, d_keys,
                       d_vers, (const uint8_t *)d_vals);
  else
    hipLaunchKernelGGL(k_load_build<128>, dim3(nb), dim3(LD_TB), 0, st, tb, (const uint32_t *)s.key_b, (const uint32_t *)s.idx_b, (const uint32_t *)s.key_a,
                       (const uint32_t *)s.idx_a, (const unsigned long long *)s.scan, (const uint32_t *)s.elist, (uint32_t)n, (uint32_t)n_ent, need, d_keys,
                       d_vers, (const uint8_t *)d_vals);
}

// rows first .. first + m - 1 as the m load requests of one pass into d_req
void dint_launch_load_msgs(const dint_kv &kv, uint32_t t, const uint64_t *d_keys, const uint32_t *d_vers, const void *d_vals, uint64_t first, uint32_t m,
                           void *d_req, hipStream_t st) {
  if (!m) return;
  hipLaunchKernelGGL(k_load_msgs, dim3(ld_blocks(m, LD_TB / 64)), dim3(LD_TB), 0, st, dint_kv_format(kv.workload), t, d_keys, d_vers, (const uint8_t *)d_vals,
                     first, m, (uint8_t *)d_req);
}

// ---- the tile tables of the two data-dependent groups: one per process, grown to the largest n seen ---------------------------
namespace {
std::mutex g_tiles_mu;
sl_tiles g_tiles[2];  // [0] ACCESS INFO, [1] SPECIAL FACILITY + CALL FORWARDING
}  // namespace
// entries 0 .. n_subs / SL_TILE of `group`'s table copied out (rows of table `which`), and the rows of exactly n_subs subscribers
int dint_load_tiles(uint32_t group, uint32_t which, uint64_t n_subs, std::vector<uint64_t> *state, std::vector<uint64_t> *rows, uint64_t *total) {
  if ((group != SL_G_AI && group != SL_G_SFCF) || which > 1) return DINT_EINVAL;
  try {
    std::lock_guard<std::mutex> lk(g_tiles_mu);
    sl_tiles &tl = g_tiles[group == SL_G_SFCF];
    sl_tile_walk(group, tl, n_subs);
    const uint64_t k = n_subs / SL_TILE;
    if (state) state->assign(tl.state.begin(), tl.state.begin() + k + 1);
    if (rows) rows->assign(tl.rows[which].begin(), tl.rows[which].begin() + k + 1);
    uint64_t g = tl.state[k], tot = tl.rows[which][k];
    for (uint64_t s = k * SL_TILE; s < n_subs; s++) {  // (the last, partial tile)
      uint32_t r[2];
      sl_skip_sub(group, s, g, r);
      tot += r[which];
    }
    if (total) *total = tot;
    return 0;
  } catch (const std::bad_alloc &) {
    return DINT_ENOMEM;
  }
}

// rows of table `which` of `group` for n_subs subscribers (the caller knows how many: cap); the tile arrays on the device for a
// data-dependent group
void dint_launch_load_gen(uint32_t group, uint32_t which, uint64_t n_subs, const uint64_t *d_tile_state, const uint64_t *d_tile_rows, uint64_t *d_keys,
                          void *d_vals, uint64_t cap, uint32_t val_size, hipStream_t st) {
  if (!n_subs) return;
  const uint32_t nb = ld_blocks(n_subs, SL_TILE);
  if (val_size == 40)
    hipLaunchKernelGGL(k_load_gen<5>, dim3(nb), dim3(LD_TB), 0, st, group, which, n_subs, d_tile_state, d_tile_rows, d_keys, (uint64_t *)d_vals, cap);
  else
    hipLaunchKernelGGL(k_load_gen<1>, dim3(nb), dim3(LD_TB), 0, st, group, which, n_subs, d_tile_state, d_tile_rows, d_keys, (uint64_t *)d_vals, cap);
}

// ---- the host forms (include/dint_driver.h) -------------------------------------------------------------------------------------
extern "C" uint32_t dint_populate_tile(void) { return SL_TILE; }

extern "C" int dint_state_load_place_host(const dint_tables_view *view, uint32_t table, const uint64_t *keys, const uint32_t *vers, const void *vals,
                                          uint64_t n, dint_load_stats *out) {
  if (out) memset(out, 0, sizeof *out);
  dint_kv kv;
  if (int rc = dint_view_kv(view, view, DINT_KV_MAX_TABLES, &kv)) return rc;
  if (table >= kv.n_tables || n > SL_MAX_ROWS || (n && (!keys || !vals))) {
    dint_set_last_error("bad table, a null array or more than 2^32 - 16 rows");
    return DINT_EINVAL;
  }
  try {
    const kv_tab &t = kv.h.tab[table];
    std::vector<uint32_t> order;
    std::vector<uint64_t> bucket;
    const sl_place_result r = sl_plan_host(keys, n, kv.hash_size[table], kv.h.shard_index, kv.h.shard_count, dint_hash_key, order, bucket);
    if (out) {
      out->rows_loaded = r.rows_loaded;
      out->foreign_rows = r.foreign_rows;
      out->table[table].rows = r.rows_loaded;
      out->table[table].overflow_entries = r.overflow_entries;
      out->table[table].longest_chain_entries = r.longest_chain_entries;
    }
    if (r.too_long) {
      dint_set_last_error("a bucket would need more than 4095 overflow entries: nothing was written");
      return DINT_ESTATE;
    }
    if (r.overflow_entries > t.pool_cap) {
      dint_set_last_error("the table needs more overflow entries than the pool has: nothing was written");
      return DINT_ENOMEM;
    }
    sl_build_host(t, keys, vers, (const uint8_t *)vals, n, order, bucket);
    if (out) out->direct = out->table[table].direct = 1;
    return 0;
  } catch (const std::bad_alloc &) {
    return DINT_ENOMEM;
  }
}

extern "C" int64_t dint_populate_tile_states_host(uint32_t workload, uint32_t table, uint64_t n_subs, uint64_t *state, uint64_t *rows, uint64_t cap) {
  uint32_t which;
  const uint32_t group = sl_group(workload, table, &which);
  if (group == SL_G_NONE) return DINT_EINVAL;
  if (sl_draws(group) != SL_DRAWS_VAR) return DINT_ESTATE;
  std::vector<uint64_t> st, ro;
  uint64_t total = 0;
  if (int rc = dint_load_tiles(group, which, n_subs, &st, &ro, &total)) return rc;
  for (uint64_t k = 0; k < st.size() && k < cap; k++) {
    if (state) state[k] = st[k];
    if (rows) rows[k] = ro[k];
  }
  return (int64_t)st.size();
}

extern "C" int64_t dint_populate_rows_host(uint32_t workload, uint32_t table, uint64_t first, uint64_t count, uint64_t *keys, void *vals, uint64_t cap) {
  uint32_t which;
  const uint32_t group = sl_group(workload, table, &which);
  if (group == SL_G_NONE || first + count < first || (cap && (!keys || !vals))) return DINT_EINVAL;
  const uint32_t vw = workload == DINT_WL_SMALLBANK ? 1u : 5u, draws = sl_draws(group);
  uint64_t g;
  if (draws == SL_DRAWS_VAR) {  // the tile table, then the draw rule alone up to `first`
    std::vector<uint64_t> st;
    if (int rc = dint_load_tiles(group, which, first, &st, nullptr, nullptr)) return rc;
    g = st.back();
    for (uint64_t s = first / SL_TILE * SL_TILE; s < first; s++) {
      uint32_t r[2];
      sl_skip_sub(group, s, g, r);
    }
  } else {
    g = sl_lcg_jump(SL_SEED, (uint64_t)draws * first);
  }
  uint64_t at = 0;
  uint8_t *out = (uint8_t *)vals;
  for (uint64_t s = first; s < first + count; s++)
    sl_gen_sub(group, s, g, [&](uint32_t w_, uint64_t key, const uint64_t *w) {
      if (w_ != which) return;
      if (at < cap) {
        keys[at] = key;
        memcpy(out + at * 8 * vw, w, 8 * vw);
      }
      at++;
    });
  return (int64_t)at;
}
