// k_locks_state.hip -- the lock units a server holds, listed where they lie, and orphaned ones released (include/dint_abi.h
// dint_state_locks / dint_state_unlock, driven by engine.hip; the rule lives in state_locks.h, which the host forms at the end of
// this file share).  Beside the hot path: no pass kernel, no pass scratch.
//
//   k_locks_units<MODE, OP>  a workgroup of 256 lanes takes one TILE of a table: lock tables 512 slots -- a lane streams two slots
//                      with one 16-byte load --, kv 256 local buckets, one lane each.  tatp reads the 16-byte link vector of the
//                      inline header (the sector that holds lockw), smallbank the two vectors of the counter pairs (the sector
//                      behind the header); the link vector of a smallbank bucket, the owner key and the chain are touched only by
//                      a lane with a held unit -- rare on a live server, so the divergent walk is the cold path.
//                        OP_COUNT  cnt[tile] = the tile's held units, part[tile] = its statistics (state_locks.h LKS_*)
//                        OP_WRITE  the tile's records: a lane's rank = the held units of the lanes below it, from one wave ballot
//                                  per unit position plus the per-wave counts in LDS, on top of the tile's offset from the scan.
//                                  A lane stores its records as 8-byte words; a tile's records leave as one run.  No atomic
//                                  decides a position: two calls write the same bytes.
//                        OP_SWEEP  DINT_UNLOCK_ALL: every held unit released (or, dry, only counted); part[tile] as OP_COUNT
//   k_state_scan       state_dev.h's one-workgroup scan over the tiles' counts, all tables in table order
//   k_locks_sum        word k of the partials summed over a range of tiles (a table): grid (LK_PART, ranges), no atomic
//   k_unlock_check     one lane per record of a list: the record and the one before it against state_locks.h lk_record_bad; the
//                      lowest refused index into words[0]
//   k_unlock_apply     reads words[0] first and does nothing for a refused list.  One lane per record: compare and release.  Two
//                      records never name one unit (the check: strictly ascending), and the four units of a tatp bucket are four
//                      bytes released by byte stores, so no lane writes what another lane's record covers.
// Nothing in a table or a list can send an access outside the tables, the scratch and the cap records: a unit is range-checked by
// lk_unit_of before it becomes an address, every chain link by its owner, every store by cap.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <cstring>

#include "../../include/dint_abi.h"
#include "../../include/dint_driver.h"
#include "dint_kernels.h"
#include "dint_kv.h"
#include "state_dev.h"
#include "state_image.h"
#include "state_locks.h"

#define LK_TB SD_TB
enum : uint32_t { OP_COUNT = 0, OP_WRITE = 1, OP_SWEEP = 2 };

struct lk_tile_args {
  kv_tab t;            // kv
  const uint2 *tbl;    // lock tables
  uint64_t n_local;    // local buckets / local slots
  uint64_t size;       // global bucket count
  dint_mod lockmod;
  uint32_t table, shard_index, shard_count, same_key;
};

template <uint32_t MODE>
struct lk_units {
  static constexpr uint32_t N = (MODE == LK_TATP || MODE == LK_SMALLBANK) ? 4u : 2u;
  uint32_t mask;
  uint32_t a[N], b[N];
};

// the units of item i of a tile's table: local bucket i (kv), local slots 2 i and 2 i + 1 (lock tables)
template <uint32_t MODE>
__device__ static inline lk_units<MODE> lk_load_units(const lk_tile_args &A, uint64_t i, sd_v4 &lv) {
  lk_units<MODE> u;
  u.mask = 0;
#pragma unroll
  for (uint32_t q = 0; q < lk_units<MODE>::N; q++) u.a[q] = u.b[q] = 0;
  if (MODE == LK_TATP) {
    if (i < A.n_local) {
      lv = *((const KV_G(sd_v4) *)kv_entry_ptr(A.t, i, KV_INLINE) + SI_LINK_VEC);
#pragma unroll
      for (uint32_t q = 0; q < 4; q++) u.a[q] = (lv.w >> (8 * q)) & 0xFFu;
    }
  } else if (MODE == LK_SMALLBANK) {
    if (i < A.n_local) {
      const KV_G(sd_v4) *p = (const KV_G(sd_v4) *)(kv_entry_ptr(A.t, i, KV_INLINE) + KV_SB_LOCK_OFF);
      const sd_v4 c0 = p[0], c1 = p[1];
      u.a[0] = c0.x; u.b[0] = c0.y; u.a[1] = c0.z; u.b[1] = c0.w;
      u.a[2] = c1.x; u.b[2] = c1.y; u.a[3] = c1.z; u.b[3] = c1.w;
    }
  } else {
    const uint64_t s0 = 2 * i;
    if (s0 + 1 < A.n_local) {
      const sd_v4 v = ((const KV_G(sd_v4) *)A.tbl)[i];
      u.a[0] = v.x; u.b[0] = v.y; u.a[1] = v.z; u.b[1] = v.w;
    } else if (s0 < A.n_local) {  // (an odd table's last slot)
      const sd_v2 v = ((const KV_G(sd_v2) *)A.tbl)[s0];
      u.a[0] = v.x; u.b[0] = v.y;
    }
  }
#pragma unroll
  for (uint32_t q = 0; q < lk_units<MODE>::N; q++)
    if (lk_held(MODE, u.a[q], u.b[q])) u.mask |= 1u << q;
  return u;
}

// what the workload's own release leaves in a unit
template <uint32_t MODE>
__device__ static inline void lk_release(const kv_tab &t, uint2 *tbl, uint64_t bucket, uint32_t q) {
  if (MODE == LK_FASST) KV_ST(uint32_t, &tbl[bucket].x, 0u);             // lock = 0, the version stays (kAbort)
  else if (MODE == LK_2PL) KV_ST(sd_v2, &tbl[bucket], ((sd_v2){0u, 0u}));
  else if (MODE == LK_SMALLBANK) KV_ST(sd_v2, kv_entry_ptr(t, bucket, KV_INLINE) + KV_SB_LOCK_OFF + 8 * q, ((sd_v2){0u, 0u}));
  else KV_ST(uint8_t, kv_entry_ptr(t, bucket, KV_INLINE) + KV_LOCKB_OFF + q, (uint8_t)0);  // one byte: its neighbours belong to other records
}

// the workgroup's partial: word k = the sum of the lanes' v[k]  (every thread calls)
__device__ static inline void lk_store_part(uint64_t (&red)[LK_TB / 64][LK_PART], const uint64_t (&v)[LK_PART], unsigned long long *part) {
#pragma unroll
  for (uint32_t k = 0; k < LK_PART; k++) {
    const uint64_t s = sd_wave_sum_u64(v[k]);
    if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < LK_PART) {
    uint64_t s = 0;
    for (uint32_t w = 0; w < LK_TB / 64; w++) s += red[w][threadIdx.x];
    part[(size_t)LK_PART * blockIdx.x + threadIdx.x] = s;
  }
}

// cnt / part / off: the table's first tile's words.  out, cap: OP_WRITE.  dry: OP_SWEEP
template <uint32_t MODE, uint32_t OP>
__global__ void __launch_bounds__(LK_TB) k_locks_units(lk_tile_args A, uint32_t *__restrict__ cnt, unsigned long long *__restrict__ part,
                                                       const uint64_t *__restrict__ off, uint64_t *__restrict__ out, uint64_t cap, uint32_t dry) {
  constexpr uint32_t N = lk_units<MODE>::N;
  constexpr bool KV = MODE == LK_TATP || MODE == LK_SMALLBANK;
  __shared__ uint64_t red[LK_TB / 64][LK_PART];
  __shared__ uint32_t wc[LK_TB / 64];
  const uint32_t tid = threadIdx.x, wave = tid >> 6;
  const uint64_t i = (uint64_t)blockIdx.x * LK_TB + tid;
  sd_v4 lv = {0u, 0u, 0u, 0u};
  const lk_units<MODE> u = lk_load_units<MODE>(A, i, lv);
  uint64_t st[LK_PART] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t before = 0, wtot = 0;
  if (OP == OP_WRITE) {
#pragma unroll
    for (uint32_t q = 0; q < N; q++) {
      const uint64_t m = __ballot((u.mask >> q) & 1u);
      before += (uint32_t)__popcll(m & lanemask_lt());
      wtot += (uint32_t)__popcll(m);
    }
    if ((tid & 63u) == 0) wc[wave] = wtot;
    __syncthreads();
    for (uint32_t w = 0; w < wave; w++) before += wc[w];
  }
  if (u.mask) {  // the cold path
    if (KV && MODE == LK_SMALLBANK && OP != OP_SWEEP) lv = *((const KV_G(sd_v4) *)kv_entry_ptr(A.t, i, KV_INLINE) + SI_LINK_VEC);
    const sd_bucket ch = {A.t, i, lv};
    uint64_t at = OP == OP_WRITE ? off[blockIdx.x] + before : 0;
#pragma unroll
    for (uint32_t q = 0; q < N; q++) {
      if (!((u.mask >> q) & 1u)) continue;
      st[LKS_HELD]++;
      st[LKS_SUM_A] += u.a[q];
      st[LKS_SUM_B] += u.b[q];
      if (OP == OP_SWEEP) {
        if (!dry) lk_release<MODE>(A.t, (uint2 *)A.tbl, KV ? i : 2 * i + q, q);
        continue;
      }
      lk_cand c = {0, 0, 0};
      if (KV) {
        c = lk_candidates(ch, ch.head(), A.lockmod, (uint64_t)q * A.size + (i * A.shard_count + A.shard_index));
        st[LKS_NO_ROW] += c.rows == 0;
        st[LKS_WALK_CUT] += (c.flags & LK_WALK_CUT) != 0;
      }
      if (OP == OP_WRITE) {
        if (at < cap) {
          const bool own = MODE == LK_TATP && A.same_key;
          const uint64_t owner = own ? KV_LD(uint64_t, kv_entry_ptr(A.t, i, KV_INLINE) + KV_OWNER_OFF + 8 * q) : 0;
          const dint_lock_record r = lk_record(A.table, KV ? (uint64_t)q * A.n_local + i : 2 * i + q, u.a[q], u.b[q], own, owner, c);
          uint64_t w[4];
          lk_record_words(r, w);
          KV_G(uint64_t) *o = (KV_G(uint64_t) *)(out + 4 * at);
          o[0] = w[0]; o[1] = w[1]; o[2] = w[2]; o[3] = w[3];
        }
        at++;
      }
    }
  }
  if (OP != OP_WRITE) {
    lk_store_part(red, st, part);
    if (OP == OP_COUNT) {
      // (the partial's first word is the tile's count: it fits 32 bits)
      if (tid == 0) {
        uint32_t c = 0;
        for (uint32_t w = 0; w < LK_TB / 64; w++) c += (uint32_t)red[w][LKS_HELD];
        cnt[blockIdx.x] = c;
      }
    }
  }
}

// out[LK_PART r + k] = word k of part[lo[r] .. hi[r]) summed: blockIdx.x = k, blockIdx.y = r
struct lk_ranges {
  uint64_t lo[LK_MAX_TABLES], hi[LK_MAX_TABLES];
};
__global__ void __launch_bounds__(LK_TB) k_locks_sum(const unsigned long long *__restrict__ part, lk_ranges r, unsigned long long *__restrict__ out) {
  __shared__ uint64_t red[LK_TB / 64];
  const uint32_t k = blockIdx.x, g = blockIdx.y;
  uint64_t s = 0;
  for (uint64_t b = r.lo[g] + threadIdx.x; b < r.hi[g]; b += LK_TB) s += part[(size_t)LK_PART * b + k];
  s = sd_wave_sum_u64(s);
  if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t v = 0;
    for (uint32_t w = 0; w < LK_TB / 64; w++) v += red[w];
    out[(size_t)LK_PART * g + k] = v;
  }
}

__device__ static inline dint_lock_record lk_load_record(const uint64_t *rec, uint64_t i) {
  const KV_G(uint64_t) *p = (const KV_G(uint64_t) *)(rec + 4 * i);
  const uint64_t w[4] = {p[0], p[1], p[2], p[3]};
  return lk_record_of_words(w);
}

// words[0] = min(words[0], the index of a record the list is refused at)
__global__ void __launch_bounds__(LK_TB) k_unlock_check(lk_geom g, const uint64_t *__restrict__ rec, uint64_t n, unsigned long long *words) {
  const uint64_t i = (uint64_t)blockIdx.x * LK_TB + threadIdx.x;
  if (i >= n) return;
  const dint_lock_record r = lk_load_record(rec, i), p = i ? lk_load_record(rec, i - 1) : r;
  if (lk_record_bad(g, r, i > 0, p)) atomicMin(words, (unsigned long long)i);
}

struct lk_apply_args {
  lk_geom g;
  kv_tab tab[LK_MAX_TABLES];
  uint2 *tbl;
};
template <uint32_t MODE>
__global__ void __launch_bounds__(LK_TB) k_unlock_apply(lk_apply_args A, const uint64_t *__restrict__ rec, uint64_t n,
                                                        const unsigned long long *words, unsigned long long *__restrict__ part, uint32_t dry) {
  constexpr bool KV = MODE == LK_TATP || MODE == LK_SMALLBANK;
  __shared__ uint64_t red[LK_TB / 64][LK_PART];
  uint64_t st[LK_PART] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool refused = *(const volatile KV_G(unsigned long long) *)words != LK_NO_INDEX;  // (the same in every lane of the grid)
  const uint64_t i = (uint64_t)blockIdx.x * LK_TB + threadIdx.x;
  if (!refused && i < n) {
    const dint_lock_record r = lk_load_record(rec, i);
    const lk_unit u = lk_unit_of(A.g, r.table, r.slot);
    if (u.ok) {  // (always, in a list that passed the check)
      const kv_tab &t = A.tab[KV ? r.table : 0];
      uint32_t a = 0, b = 0;
      bool same_owner = true;
      if (MODE == LK_TATP) {
        const uint8_t *ie = kv_entry_ptr(t, u.bucket, KV_INLINE);
        a = KV_LD(uint8_t, ie + KV_LOCKB_OFF + u.q);
        if (A.g.same_key && (r.flags & LK_KEY_OWNER)) same_owner = KV_LD(uint64_t, ie + KV_OWNER_OFF + 8 * u.q) == r.key;
      } else if (MODE == LK_SMALLBANK) {
        const sd_v2 v = KV_LD(sd_v2, kv_entry_ptr(t, u.bucket, KV_INLINE) + KV_SB_LOCK_OFF + 8 * u.q);
        a = v.x; b = v.y;
      } else {
        const sd_v2 v = KV_LD(sd_v2, &A.tbl[u.bucket]);
        a = v.x; b = v.y;
      }
      if (lk_held(MODE, a, b) && lk_same(MODE, a, b, r.a, r.b) && same_owner) {
        if (!dry) lk_release<MODE>(t, A.tbl, u.bucket, u.q);
#pragma unroll
        for (uint32_t k = 0; k < LK_MAX_TABLES; k++) st[LKU_TABLE + k] += r.table == k;  // (no runtime-indexed array of the lane)
        st[LKU_REL_A] = a;
        st[LKU_REL_B] = MODE == LK_FASST ? 0 : b;
      } else {
        st[LKU_STALE] = 1;
      }
    }
  }
  lk_store_part(red, st, part);
}

// ------------------------------------------------------------------------------------------------------ host side
static inline uint64_t lk_table_tiles(const lk_geom &g, uint32_t t) {
  const uint64_t items = lk_is_kv(g.mode) ? g.n_local[t] : (g.n_local[t] + 1) / 2;
  const uint64_t nb = (items + LK_TB - 1) / LK_TB;
  return nb ? nb : 1;
}
uint64_t dint_locks_blocks(const dint_locks_view &v) {
  uint64_t nb = 0;
  for (uint32_t t = 0; t < v.g.n_tables; t++) nb += lk_table_tiles(v.g, t);
  return nb;
}
uint64_t dint_locks_list_blocks(uint64_t n) { return (n + LK_TB - 1) / LK_TB; }

static lk_tile_args lk_tile_of(const dint_locks_view &v, uint32_t t) {
  lk_tile_args A;
  memset(&A, 0, sizeof A);
  if (lk_is_kv(v.g.mode)) A.t = v.tab[t];
  A.tbl = v.tbl;
  A.n_local = v.g.n_local[t];
  A.size = v.g.size[t];
  A.lockmod = v.lockmod[t];
  A.table = t; A.shard_index = v.g.shard_index; A.shard_count = v.g.shard_count; A.same_key = v.g.same_key;
  return A;
}
template <uint32_t OP>
static void lk_launch_units(const dint_locks_view &v, const dint_locks_scratch &s, uint64_t *out, uint64_t cap, uint32_t dry, hipStream_t st) {
  uint64_t base = 0;
  for (uint32_t t = 0; t < v.g.n_tables; t++) {
    const lk_tile_args A = lk_tile_of(v, t);
    const uint32_t grid = (uint32_t)lk_table_tiles(v.g, t);
    uint32_t *cnt = s.cnt + base;
    unsigned long long *part = s.part + (size_t)LK_PART * base;
    const uint64_t *off = s.off + base;
    switch (v.g.mode) {
      case LK_FASST: hipLaunchKernelGGL((k_locks_units<LK_FASST, OP>), dim3(grid), dim3(LK_TB), 0, st, A, cnt, part, off, out, cap, dry); break;
      case LK_2PL: hipLaunchKernelGGL((k_locks_units<LK_2PL, OP>), dim3(grid), dim3(LK_TB), 0, st, A, cnt, part, off, out, cap, dry); break;
      case LK_TATP: hipLaunchKernelGGL((k_locks_units<LK_TATP, OP>), dim3(grid), dim3(LK_TB), 0, st, A, cnt, part, off, out, cap, dry); break;
      default: hipLaunchKernelGGL((k_locks_units<LK_SMALLBANK, OP>), dim3(grid), dim3(LK_TB), 0, st, A, cnt, part, off, out, cap, dry); break;
    }
    base += grid;
  }
}
static void lk_launch_table_sums(const dint_locks_view &v, const dint_locks_scratch &s, hipStream_t st) {
  lk_ranges r;
  memset(&r, 0, sizeof r);
  uint64_t base = 0;
  for (uint32_t t = 0; t < v.g.n_tables; t++) {
    r.lo[t] = base;
    base += lk_table_tiles(v.g, t);
    r.hi[t] = base;
  }
  hipLaunchKernelGGL(k_locks_sum, dim3(LK_PART, v.g.n_tables), dim3(LK_TB), 0, st, (const unsigned long long *)s.part, r, s.words + DINT_LOCKS_SUMS_AT);
}

void dint_launch_locks_list(const dint_locks_view &v, dint_locks_scratch s, void *d_records, uint64_t cap, hipStream_t st) {
  lk_launch_units<OP_COUNT>(v, s, nullptr, 0, 0, st);
  sd_launch_scan((const uint32_t *)s.cnt, (uint32_t)dint_locks_blocks(v), s.off, s.words + 1, st);
  lk_launch_table_sums(v, s, st);
  if (d_records && cap) lk_launch_units<OP_WRITE>(v, s, (uint64_t *)d_records, cap, 0, st);
}

void dint_launch_locks_sweep(const dint_locks_view &v, dint_locks_scratch s, bool dry, hipStream_t st) {
  lk_launch_units<OP_SWEEP>(v, s, nullptr, 0, dry ? 1u : 0u, st);
  lk_launch_table_sums(v, s, st);
}

void dint_launch_locks_release(const dint_locks_view &v, dint_locks_scratch s, const void *d_records, uint64_t n, bool dry, hipStream_t st) {
  const uint32_t grid = (uint32_t)dint_locks_list_blocks(n);
  (void)hipMemsetAsync(s.words, 0xFF, sizeof(unsigned long long), st);  // words[0] = LK_NO_INDEX
  hipLaunchKernelGGL(k_unlock_check, dim3(grid), dim3(LK_TB), 0, st, v.g, (const uint64_t *)d_records, n, s.words);
  lk_apply_args A;
  memset(&A, 0, sizeof A);
  A.g = v.g;
  if (lk_is_kv(v.g.mode))
    for (uint32_t t = 0; t < v.g.n_tables; t++) A.tab[t] = v.tab[t];
  A.tbl = v.tbl;
  const uint64_t *rec = (const uint64_t *)d_records;
  const unsigned long long *w = s.words;
  const uint32_t d = dry ? 1u : 0u;
  switch (v.g.mode) {
    case LK_FASST: hipLaunchKernelGGL(k_unlock_apply<LK_FASST>, dim3(grid), dim3(LK_TB), 0, st, A, rec, n, w, s.part, d); break;
    case LK_2PL: hipLaunchKernelGGL(k_unlock_apply<LK_2PL>, dim3(grid), dim3(LK_TB), 0, st, A, rec, n, w, s.part, d); break;
    case LK_TATP: hipLaunchKernelGGL(k_unlock_apply<LK_TATP>, dim3(grid), dim3(LK_TB), 0, st, A, rec, n, w, s.part, d); break;
    default: hipLaunchKernelGGL(k_unlock_apply<LK_SMALLBANK>, dim3(grid), dim3(LK_TB), 0, st, A, rec, n, w, s.part, d); break;
  }
  lk_ranges r;
  memset(&r, 0, sizeof r);
  r.hi[0] = grid;
  hipLaunchKernelGGL(k_locks_sum, dim3(LK_PART, 1), dim3(LK_TB), 0, st, (const unsigned long long *)s.part, r, s.words + DINT_LOCKS_SUMS_AT);
}

// ---- the host forms (include/dint_driver.h): the same state_locks.h rule over memory of the caller -----------------------------
extern "C" int64_t dint_state_locks_image_host(const void *image, uint64_t bytes, dint_lock_record *records, uint64_t cap, dint_lock_stats *out) {
  if (!records && cap) {
    dint_set_last_error("no room for cap records");
    return DINT_EINVAL;
  }
  if (int rc = dint_state_image_check_host(image, bytes)) return rc;
  si_header h;
  memcpy(&h, image, sizeof h);
  const uint32_t mode = lk_mode(h.workload);
  if (mode == LK_NONE) {
    dint_set_last_error("workload has no lock table");
    return DINT_ESTATE;
  }
  const bool lock = h.stride == SI_LOCK_STRIDE, same_key = mode == LK_TATP && (h.flags & DINT_FLAG_LOCK_SAME_KEY);
  dint_lock_stats s;
  memset(&s, 0, sizeof s);
  uint8_t *dst = (uint8_t *)records;
  auto emit = [&](const dint_lock_record &r) {
    if (s.total < cap) memcpy(dst + s.total * sizeof r, &r, sizeof r);
    s.total++;
    s.held[r.table]++;
    s.sum_a += r.a;
    s.sum_b += r.b;
  };
  for (uint32_t t = 0; t < h.n_tables; t++) {
    const si_host_image im(h, t, (const uint8_t *)image, lock);
    const uint64_t n_local = lk_n_local(h.table[t].global_size, h.src_count);
    const dint_mod lockmod = dint_make_mod(4 * h.table[t].global_size);
    for (uint64_t b = 0; b < h.table[t].n_buckets; b++) {
      const si_dir d = im.dir(b);
      const uint64_t l = d.id / h.src_count;
      if (lock) {  // (a slot's two words lie in its directory entry)
        if (lk_held(mode, d.first, d.count)) emit(lk_record(t, l, d.first, d.count, false, 0, lk_cand{0, 0, 0}));
        continue;
      }
      const uint8_t *inl = im.entry(b, KV_INLINE);
      for (uint32_t q = 0; q < 4; q++) {
        const uint32_t a = mode == LK_TATP ? inl[KV_LOCKB_OFF + q] : si_ld32(inl + KV_SB_LOCK_OFF + 8 * q);
        const uint32_t bb = mode == LK_TATP ? 0 : si_ld32(inl + KV_SB_LOCK_OFF + 8 * q + 4);
        if (!lk_held(mode, a, bb)) continue;
        uint32_t bad = 0;  // (the check has judged every link already: stays 0)
        const si_image_chain<si_host_image> ch = {im, b, d, &bad};
        const lk_cand c = lk_candidates(ch, ch.head(), lockmod, (uint64_t)q * h.table[t].global_size + d.id);
        s.no_row += c.rows == 0;
        s.walk_cut += (c.flags & LK_WALK_CUT) != 0;
        emit(lk_record(t, (uint64_t)q * n_local + l, a, bb, same_key, same_key ? si_ld64(inl + KV_OWNER_OFF + 8 * q) : 0, c));
      }
    }
  }
  if (out) memcpy(out, &s, sizeof s);
  return (int64_t)(s.total < cap ? s.total : cap);
}

extern "C" uint64_t dint_state_unlock_check_host(uint32_t workload, const dint_lock_geometry *geometry, const dint_lock_record *records, uint64_t n) {
  lk_geom g;
  memset(&g, 0, sizeof g);
  g.mode = lk_mode(workload);
  if (!geometry || !records || g.mode == LK_NONE) return 0;
  g.shard_count = geometry->shard_count ? geometry->shard_count : 1;
  g.shard_index = geometry->shard_index;
  g.n_tables = geometry->n_tables > LK_MAX_TABLES ? LK_MAX_TABLES : geometry->n_tables;
  for (uint32_t t = 0; t < g.n_tables; t++) {
    g.size[t] = geometry->size[t];
    g.n_local[t] = lk_n_local(g.size[t], g.shard_count);
  }
  const uint8_t *src = (const uint8_t *)records;
  dint_lock_record p, r;
  memset(&p, 0, sizeof p);
  for (uint64_t i = 0; i < n; i++) {
    memcpy(&r, src + i * sizeof r, sizeof r);
    if (lk_record_bad(g, r, i > 0, p)) return i;
    p = r;
  }
  return n;
}
