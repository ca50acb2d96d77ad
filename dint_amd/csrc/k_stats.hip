// k_stats.hip -- occupancy and chain shape of an engine's tables, read where they lie (include/dint_abi.h dint_state_stats,
// driven by engine.hip; the rule lives in state_stats.h, which the host form at the end of this file shares).
//
//   k_state_stats      one lane per bucket, the workgroups striding over the table (DINT_STATE_STATS_GRID at most).  A lane
//                      loads the 16-byte link vector of the inline header and walks the chain from it (state_dev.h sd_bucket
//                      under state_image.h si_chain_walk): header sectors only, 8 bytes {validw, next} per overflow entry, values never.  Key vectors are
//                      loaded only by a bucket of more than one valid slot, for the duplicate comparison, which re-walks (no
//                      per-lane array).  The counters stay in registers until the workgroup has run out of buckets; the two
//                      histograms go to one LDS array per WAVE -- the lanes that share a bin are found with a ballot and one
//                      of them adds their number, so there is no atomic, not even in LDS.  The workgroup then stores ONE
//                      partial report of ST_WORDS words, thread w word w.
//   k_state_stats_sum  one workgroup per table adds up the partials (k_state_digest_sum's shape): sums, two maxima, and for
//                      longest_chain_bucket the (longest chain, then lowest id) pair.  No atomics, no order dependence.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <cstdio>
#include <cstring>

#include "../../include/dint_abi.h"
#include "../../include/dint_driver.h"
#include "dint_kernels.h"
#include "dint_kv.h"
#include "state_dev.h"
#include "state_image.h"
#include "state_stats.h"

#define ST_TB SD_TB      // threads per workgroup of k_state_stats
#define ST_SUM_TB 1024u  // ... of k_state_stats_sum: 8 groups of 128 threads, thread w of a group word w
#define ST_GRID DINT_STATE_STATS_GRID

static_assert(ST_WORDS == DINT_STATE_STATS_WORDS && sizeof(dint_table_stats) == 8 * ST_WORDS, "a report is a dint_table_stats");
static_assert(offsetof(dint_table_stats, chain_hist) == 8 * ST_CHAIN_HIST && offsetof(dint_table_stats, rows_hist) == 8 * ST_ROWS_HIST &&
              offsetof(dint_table_stats, reserved) == 8 * ST_BAD && offsetof(dint_table_stats, pool_top) == 8 * ST_POOL_TOP &&
              offsetof(dint_table_stats, longest_chain_bucket) == 8 * ST_LONGEST_BUCKET && offsetof(dint_table_stats, locks_held) == 8 * ST_LOCKS,
              "the words of state_stats.h are the fields of dint_table_stats");

// h[bin] += the active lanes of this wave that hold `bin` (h: this wave's own LDS array; every lane of the wave calls).  One
// round per distinct bin among the lanes -- mostly one or two: neighbouring buckets look alike.
typedef __attribute__((address_space(3))) uint32_t st_lds_u32;  // (an LDS access the compiler knows is one: ds_, not flat_)
__device__ static inline void st_hist_add(st_lds_u32 *h, uint32_t bin, bool active) {
  uint64_t todo = __ballot(active);
  while (todo) {
    const uint32_t leader = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
    const uint32_t v = (uint32_t)__shfl((int)bin, (int)leader, 64);
    const uint64_t same = __ballot(active && bin == v);
    if ((threadIdx.x & 63u) == leader) h[v] += (uint32_t)__popcll(same);
    todo &= ~same;
  }
}

// the sums a lane keeps, in the order they are reduced (red[wave][k]); then the maxima
enum : uint32_t { SL_BUCKETS = 0, SL_EMPTY, SL_ROWS, SL_ENTRIES, SL_OVERFLOW, SL_FIRST, SL_UNLINKED, SL_HIT, SL_SHADOWED, SL_UNCHECKED,
                  SL_LOCKS, SL_BAD, SL_SUMS, SL_LONGEST = SL_SUMS, SL_LONGEST_ID, SL_MOST, SL_N };

// lock_mode: state_image.h SI_LOCKS_*
// part[ST_WORDS * workgroup ..] = the report of the buckets this workgroup walked (state_stats.h words; holes and the pool words 0)
__global__ void __launch_bounds__(ST_TB) k_state_stats(kv_tab t, uint32_t lock_mode, uint32_t shard_index, uint32_t shard_count,
                                                       unsigned long long *__restrict__ part) {
  __shared__ uint32_t hist[ST_TB / 64][ST_CHAIN_BINS + ST_ROWS_BINS];
  __shared__ uint64_t red[ST_TB / 64][SL_N];
  __shared__ uint64_t fin[ST_WORDS];
  const uint32_t tid = threadIdx.x, wave = tid >> 6;
  if (tid < ST_CHAIN_BINS + ST_ROWS_BINS) {
#pragma unroll
    for (uint32_t w = 0; w < ST_TB / 64; w++) hist[w][tid] = 0;
  }
  if (tid < ST_WORDS) fin[tid] = 0;
  __syncthreads();
  uint32_t n_b = 0, empty = 0, rows = 0, entries = 0, overflow = 0, first = 0, unlinked = 0, shadowed = 0, unchecked = 0, locks = 0, bad = 0;
  uint64_t hit = 0, longest_id = ST_NO_BUCKET;
  uint32_t longest = 0, most = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * ST_TB; base < t.n_local; base += (uint64_t)gridDim.x * ST_TB) {  // (uniform in the workgroup)
    const uint64_t b = base + tid;
    const bool active = b < t.n_local;
    uint32_t cbin = 0, rbin = 0;
    bool counted = false;
    if (active) {
      const sd_bucket ch = sd_bucket_at(t, b);
      const st_bucket r = st_bucket_walk(ch);
      n_b++;
      locks += ch.locks_held(lock_mode);
      counted = r.ok;
      if (r.ok) {
        empty += r.rows == 0;
        rows += r.rows;
        entries += r.entries;
        overflow += r.overflow;
        first += r.first;
        unlinked += r.entries != 0 && !r.linked;
        hit += r.hit;
        shadowed += r.shadowed;
        unchecked += r.unchecked;
        const uint64_t id = b * shard_count + shard_index;
        if (r.entries && st_longer(r.entries, id, longest, longest_id)) {
          longest = r.entries;
          longest_id = id;
        }
        most = max(most, r.rows);
        cbin = st_chain_bin(r.entries);
        rbin = st_rows_bin(r.rows);
      } else {
        bad++;
      }
    }
    st_hist_add((st_lds_u32 *)hist[wave], cbin, counted);
    st_hist_add((st_lds_u32 *)hist[wave] + ST_CHAIN_BINS, rbin, counted);
  }
  // the wave, then the workgroup
  const uint64_t s[SL_SUMS] = {n_b, empty, rows, entries, overflow, first, unlinked, hit, shadowed, unchecked, locks, bad};
  uint64_t ws[SL_SUMS];
#pragma unroll
  for (uint32_t k = 0; k < SL_SUMS; k++) ws[k] = sd_wave_sum_u64(s[k]);
  most = sd_wave_max_u32(most);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const uint32_t oc = __shfl_xor(longest, d, 64);
    const uint64_t oi = sd_shfl_xor_u64(longest_id, d);
    if (st_longer(oc, oi, longest, longest_id)) {
      longest = oc;
      longest_id = oi;
    }
  }
  if ((tid & 63u) == 0) {
#pragma unroll
    for (uint32_t k = 0; k < SL_SUMS; k++) red[wave][k] = ws[k];
    red[wave][SL_LONGEST] = longest;
    red[wave][SL_LONGEST_ID] = longest_id;
    red[wave][SL_MOST] = most;
  }
  __syncthreads();
  if (tid == 0) {
    uint64_t a[SL_N];
#pragma unroll
    for (uint32_t k = 0; k < SL_N; k++) a[k] = red[0][k];
    for (uint32_t w = 1; w < ST_TB / 64; w++) {
#pragma unroll
      for (uint32_t k = 0; k < SL_SUMS; k++) a[k] += red[w][k];
      if (st_longer(red[w][SL_LONGEST], red[w][SL_LONGEST_ID], a[SL_LONGEST], a[SL_LONGEST_ID])) {
        a[SL_LONGEST] = red[w][SL_LONGEST];
        a[SL_LONGEST_ID] = red[w][SL_LONGEST_ID];
      }
      a[SL_MOST] = a[SL_MOST] > red[w][SL_MOST] ? a[SL_MOST] : red[w][SL_MOST];
    }
    fin[ST_BUCKETS] = a[SL_BUCKETS]; fin[ST_EMPTY] = a[SL_EMPTY]; fin[ST_ROWS] = a[SL_ROWS]; fin[ST_ENTRIES] = a[SL_ENTRIES];
    fin[ST_OVERFLOW] = a[SL_OVERFLOW]; fin[ST_INLINE_FIRST] = a[SL_FIRST]; fin[ST_INLINE_UNLINKED] = a[SL_UNLINKED];
    fin[ST_HIT] = a[SL_HIT]; fin[ST_SHADOWED] = a[SL_SHADOWED]; fin[ST_UNCHECKED] = a[SL_UNCHECKED]; fin[ST_LOCKS] = a[SL_LOCKS];
    fin[ST_BAD] = a[SL_BAD]; fin[ST_LONGEST] = a[SL_LONGEST]; fin[ST_LONGEST_BUCKET] = a[SL_LONGEST_ID]; fin[ST_MOST_ROWS] = a[SL_MOST];
  }
  __syncthreads();
  if (tid < ST_WORDS) {
    uint64_t v = fin[tid];
    if (tid >= ST_CHAIN_HIST && tid < ST_BAD) {
#pragma unroll
      for (uint32_t w = 0; w < ST_TB / 64; w++) v += hist[w][tid - ST_CHAIN_HIST];
    }
    part[(size_t)ST_WORDS * blockIdx.x + tid] = v;
  }
}

// out[ST_WORDS t ..] = the partials of table t (workgroup = table) combined; n[t] of them at part + ST_WORDS * ST_GRID * t
struct st_sum_args {
  uint32_t n[DINT_KV_MAX_TABLES];
  uint32_t pool_cap[DINT_KV_MAX_TABLES];
  const uint32_t *pool_top[DINT_KV_MAX_TABLES];
};
__global__ void __launch_bounds__(ST_SUM_TB) k_state_stats_sum(const unsigned long long *__restrict__ part, st_sum_args a,
                                                               unsigned long long *__restrict__ out) {
  constexpr uint32_t G = ST_SUM_TB / 128;
  __shared__ uint64_t red[G][128], redc[G];
  const uint32_t tid = threadIdx.x, table = blockIdx.x, w = tid & 127u, g = tid >> 7;
  const unsigned long long *p = part + (size_t)ST_WORDS * ST_GRID * table;
  const uint32_t n = a.n[table];
  const bool is_max = w == ST_LONGEST || w == ST_MOST_ROWS, is_id = w == ST_LONGEST_BUCKET;
  uint64_t v = is_id ? ST_NO_BUCKET : 0, best = 0;
  if (w < ST_WORDS) {
#pragma unroll 4
    for (uint32_t k = g; k < n; k += G) {
      const uint64_t x = p[(size_t)ST_WORDS * k + w];
      if (is_id) {
        const uint64_t c = p[(size_t)ST_WORDS * k + ST_LONGEST];
        if (st_longer(c, x, best, v)) { best = c; v = x; }
      } else if (is_max) {
        v = v > x ? v : x;
      } else {
        v += x;
      }
    }
  }
  red[g][w] = v;
  if (is_id) redc[g] = best;
  __syncthreads();
  if (tid < ST_WORDS) {
    for (uint32_t k = 1; k < G; k++) {
      const uint64_t x = red[k][tid];
      if (is_id) {
        if (st_longer(redc[k], x, best, v)) { best = redc[k]; v = x; }
      } else if (is_max) {
        v = v > x ? v : x;
      } else {
        v += x;
      }
    }
    if (tid == ST_POOL_TOP) {  // (a failed insert may have left it above the pool's size for a moment)
      const uint32_t top = *(const volatile KV_G(uint32_t) *)a.pool_top[table];
      v = top < a.pool_cap[table] ? top : a.pool_cap[table];
    }
    out[(size_t)ST_WORDS * table + tid] = v;
  }
}

// ------------------------------------------------------------------------------------------------------ host side
void dint_launch_state_stats(const dint_kv &kv, dint_stats_scratch s, hipStream_t st) {
  const uint32_t lock_mode = si_lock_mode(kv.workload);
  st_sum_args a;
  memset(&a, 0, sizeof a);
  for (uint32_t t = 0; t < kv.n_tables; t++) {
    const kv_tab &tb = kv.h.tab[t];
    const uint64_t nb = (tb.n_local + ST_TB - 1) / ST_TB;
    const uint32_t grid = (uint32_t)(nb < 1 ? 1 : nb > ST_GRID ? ST_GRID : nb);
    a.n[t] = grid;
    a.pool_cap[t] = tb.pool_cap;
    a.pool_top[t] = tb.pool_top;
    hipLaunchKernelGGL(k_state_stats, dim3(grid), dim3(ST_TB), 0, st, tb, lock_mode, kv.h.shard_index, kv.h.shard_count,
                       s.part + (size_t)ST_WORDS * ST_GRID * t);
  }
  hipLaunchKernelGGL(k_state_stats_sum, dim3(kv.n_tables), dim3(ST_SUM_TB), 0, st, (const unsigned long long *)s.part, a, s.out);
}

// ---- the host form (include/dint_driver.h): the same state_stats.h rule over an image in host memory -----------------------
extern "C" int dint_state_stats_image_host(const void *image, uint64_t bytes, dint_table_stats *out, uint32_t cap_tables) {
  if (!out) {
    dint_set_last_error("null argument");
    return DINT_EINVAL;
  }
  if (int rc = dint_state_image_check_host(image, bytes)) return rc;
  si_header h;
  memcpy(&h, image, sizeof h);
  char msg[160];
  if (h.stride == SI_LOCK_STRIDE) {
    dint_set_last_error("the image of a lock table: no keys, no chains");
    return DINT_ESTATE;
  }
  if (cap_tables < h.n_tables) {
    snprintf(msg, sizeof msg, "%u tables, room for %u", h.n_tables, cap_tables);
    dint_set_last_error(msg);
    return DINT_EINVAL;
  }
  const uint32_t lock_mode = si_lock_mode(h.workload);
  for (uint32_t t = 0; t < h.n_tables; t++) {
    const si_host_image im(h, t, (const uint8_t *)image, false);
    uint64_t w[ST_WORDS];
    st_report_init(w);
    for (uint64_t b = 0; b < h.table[t].n_buckets; b++) {
      uint32_t bad = 0;  // (the check has judged every link already: stays 0)
      const si_image_chain<si_host_image> ch = {im, b, im.dir(b), &bad};
      const uint8_t *inl = im.entry(b, KV_INLINE);
      const uint32_t locks = si_locks_held(lock_mode, si_ld32(inl + KV_LOCKB_OFF), [inl](uint32_t c[8]) {
        for (uint32_t k = 0; k < 8; k++) c[k] = si_ld32(inl + KV_SB_LOCK_OFF + 4 * k);
      });
      st_report_add(w, st_bucket_walk(ch), ch.d.id, locks);
    }
    if (st_report_finish(w, 0)) {  // (the check has walked every chain already: never taken)
      snprintf(msg, sizeof msg, "a chain of table %u cannot be walked", t);
      dint_set_last_error(msg);
      return DINT_ESTATE;
    }
    memcpy(&out[t], w, sizeof w);
  }
  return (int)h.n_tables;
}
