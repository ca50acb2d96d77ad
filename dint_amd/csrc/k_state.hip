// k_state.hip -- the rows of two engines compared and one made equal to the other without leaving the GPU
// (include/dint_abi.h dint_state_digest / dint_state_diff / dint_state_repair, driven by engine.hip; the rules live in
// state_sync.h, which the host forms at the end of this file share).
//
//   k_state_digest        a stream over the entries of one table, FLAT: the inline entries and the pool entries handed out so
//                         far ([0, *pool_top)), whatever chain they hang in.  A slot is counted iff its valid byte is set: every
//                         insert and delete goes through kv_apply (dint_kv_core.h), which clears the byte BEFORE it unlinks an
//                         emptied entry and frees only emptied entries, so no unlinked or freed entry holds a valid slot
//                         (DESIGN.md "State sync").  A workgroup reads a tile of 16 KB as 16-byte vectors (16 lanes per 256-byte
//                         entry, 8 per 128-byte entry, consecutive lanes consecutive vectors) into LDS, then every thread hashes
//                         the slots of the tile from LDS; {rows, sum, xor} are reduced in the wave and in the workgroup, and a
//                         workgroup that has run out of tiles stores ONE partial.  (A first version left with one atomic per wave
//                         and word: 16,000 waves x 3 atomics on three addresses took 3.0 ms for 1.17 GB -- the atomics, not the
//                         stream.)
//   k_state_digest_sum    one workgroup per table adds up the workgroups' partials: no atomics, no order dependence
//   k_state_diff_count    one lane per bucket, the same bucket of both engines (same hash, same bucket count): the records the
//                         bucket contributes, by kind.  Fast path: the two inline headers equal in keys, versions, valid bytes
//                         and links, no overflow entry, the valid slots' values equal -> nothing, and no chain walk.  Otherwise
//                         state_sync.h ss_bucket_diff over two chain walkers.  Per workgroup one count.
//   k_state_scan          (state_dev.h) exclusive scan of the workgroup counts of all tables (table order, bucket order) on the device
//   k_state_diff_write    (launched only when there is something to write: the host has read the total by then, so two engines in
//                         sync cost ONE pass over their buckets)  the count again, a scan inside the workgroup, and the buckets
//                         that have records walk a second time and store them: ascending table, ascending bucket, a's rows in a's chain order, then b-only rows in b's
//   k_state_repair_check  records grouped by bucket? (table, bucket) non-decreasing, table in range
//   k_state_repair        the first record of every (table, bucket) run owns the bucket and applies the run in order: no two
//                         lanes ever touch one chain; buckets meet in the pool allocator only, which is atomic
// Every chain walk counts to KV_MAX_CHAIN and checks its links against the pool's size.  The diff's cursor (ss_chain) is NOT the
// walk of state_image.h si_chain_walk: it ends quietly at a bad link, and its positions are link << 2 | slot -- the repair
// relies on both.  Wave and workgroup helpers, the vector type and the scan kernel are state_dev.h's.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <numeric>
#include <vector>

#include "../../include/dint_abi.h"
#include "../../include/dint_driver.h"
#include "dint_kernels.h"
#include "dint_kv.h"
#include "state_dev.h"
#include "state_sync.h"

#define SS_TB SD_TB           // threads per workgroup, every kernel here
#define SS_TILE_VEC 1024u     // digest: 16-byte vectors per tile (16 KB)
#define SS_LDS_PAD 16u        // digest: bytes between entries in LDS (an entry's header would start in bank 0 otherwise)
#define SS_DIGEST_GRID DINT_STATE_DIGEST_GRID  // digest: workgroups at most (8 per compute unit: what the LDS tiles let stay resident)

// device-scope RMWs on the pool words, as the kv kernels (k_kv_dev.h kv_dev_mem)
struct ss_dev_mem {
  __device__ static inline uint32_t fetch_add(uint32_t *p, uint32_t v) { return atomicAdd(p, v); }
  __device__ static inline uint32_t load32(uint32_t *p) { return atomicAdd(p, 0u); }
  __device__ static inline void store32(uint32_t *p, uint32_t v) { atomicExch(p, v); }
  __device__ static inline unsigned long long load64(unsigned long long *p) { return atomicAdd(p, 0ull); }
  __device__ static inline bool cas64(unsigned long long *p, unsigned long long exp, unsigned long long des) {
    return atomicCAS(p, exp, des) == exp;
  }
};

// ------------------------------------------------------------------------------------------------------ digest
// STRIDE = bytes per entry (256: 40-byte values, 128: 8-byte values).  part[4 * workgroup ..] = {rows, sum, xor, 0} of what
// this workgroup read.
template <uint32_t STRIDE>
__global__ void __launch_bounds__(SS_TB) k_state_digest(kv_tab t, uint32_t table, unsigned long long *__restrict__ part) {
  constexpr uint32_t VPE = STRIDE / 16;             // vectors per entry
  constexpr uint32_t EPT = SS_TILE_VEC / VPE;       // entries per tile
  constexpr uint32_t LSTRIDE = STRIDE + SS_LDS_PAD; // an entry's distance in LDS
  constexpr uint32_t VS = STRIDE == 256 ? 40u : 8u;
  __shared__ sd_v4 Lv[EPT * LSTRIDE / 16];
  __shared__ uint64_t red[SS_TB / 64][3];
  const uint8_t *L = (const uint8_t *)Lv;
  const uint32_t tid = threadIdx.x;
  const uint32_t top = *(const volatile uint32_t *)t.pool_top;  // (a failed insert may have left it above the pool's size for a moment)
  const uint64_t n_ent = t.n_local + (uint64_t)(top < t.pool_cap ? top : t.pool_cap);
  const uint64_t n_vec = n_ent * VPE, n_tiles = (n_ent + EPT - 1) / EPT;
  const KV_G(sd_v4) *src = (const KV_G(sd_v4) *)t.entries;
  ss_digest d = {0, 0, 0};
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t v0 = tile * SS_TILE_VEC;
    sd_v4 v[SS_TILE_VEC / SS_TB];
#pragma unroll
    for (uint32_t k = 0; k < SS_TILE_VEC / SS_TB; k++) {
      const uint64_t g = v0 + k * SS_TB + tid;
      v[k] = g < n_vec ? __builtin_nontemporal_load(src + g) : (sd_v4)(0u);
    }
#pragma unroll
    for (uint32_t k = 0; k < SS_TILE_VEC / SS_TB; k++) {
      const uint32_t i = k * SS_TB + tid;
      Lv[(i / VPE) * (LSTRIDE / 16) + (i % VPE)] = v[k];
    }
    __syncthreads();
    for (uint32_t r = tid; r < EPT * 4; r += SS_TB) {
      const uint8_t *e = L + (r >> 2) * LSTRIDE;
      const uint32_t s = r & 3;
      if (e[KV_VALID_OFF + s]) {  // (entries beyond the table came in as zeros)
        const uint64_t *val = (const uint64_t *)(e + KV_VAL_OFF + s * VS);
        ss_digest_add(d, ss_row_hash(*(const uint64_t *)(e + 8 * s), *(const uint32_t *)(e + 32 + 4 * s), table, VS,
                                     [val](uint32_t k) { return val[k]; }));
      }
    }
    __syncthreads();
  }
  const ss_digest w = ss_block_digest(red, d);
  if (tid == 0) {
    unsigned long long *o = part + 4 * (size_t)blockIdx.x;
    o[0] = w.rows; o[1] = w.sum; o[2] = w.xr; o[3] = 0;
  }
}
// out[4 t ..] = the partials of table t (workgroup = table) combined; n[t] of them at part + 4 * SS_DIGEST_GRID * t
struct ss_digest_counts {
  uint32_t n[DINT_KV_MAX_TABLES];
};
__global__ void __launch_bounds__(SS_TB) k_state_digest_sum(const unsigned long long *__restrict__ part, ss_digest_counts cnt,
                                                            unsigned long long *__restrict__ out) {
  __shared__ uint64_t red[SS_TB / 64][3];
  const uint32_t tid = threadIdx.x, table = blockIdx.x;
  const unsigned long long *p = part + (size_t)4 * SS_DIGEST_GRID * table;
  ss_digest d = {0, 0, 0};
  for (uint32_t k = tid; k < cnt.n[table]; k += SS_TB) ss_digest_merge(d, ss_digest{p[4 * k], p[4 * k + 1], p[4 * k + 2]});
  const ss_digest w = ss_block_digest(red, d);
  if (tid == 0) {
    out[4 * table] = w.rows; out[4 * table + 1] = w.sum; out[4 * table + 2] = w.xr; out[4 * table + 3] = 0;
  }
}
static_assert(offsetof(kv_hdr, key) == 0 && offsetof(kv_hdr, ver) == 32 && offsetof(kv_hdr, validw) == KV_VALID_OFF, "header layout");

// ------------------------------------------------------------------------------------------------------ diff
// (the chain cursor ss_chain, SS_WALK_BOUND and the two emitters are state_dev.h's: k_block.hip walks the same way)

// nothing to say about bucket b without walking a chain?
template <uint32_t VS>
__device__ static inline bool ss_bucket_equal_fast(const kv_tab &ta, const kv_tab &tb, uint64_t b) {
  const uint8_t *ea = kv_entry_ptr(ta, b, KV_INLINE), *eb = kv_entry_ptr(tb, b, KV_INLINE);
  const KV_G(sd_v4) *pa = (const KV_G(sd_v4) *)ea, *pb = (const KV_G(sd_v4) *)eb;
  const sd_v4 a0 = pa[0], a1 = pa[1], a2 = pa[2], a3 = pa[3], b0 = pb[0], b1 = pb[1], b2 = pb[2], b3 = pb[3];
  const uint32_t d = (a0.x ^ b0.x) | (a0.y ^ b0.y) | (a0.z ^ b0.z) | (a0.w ^ b0.w) | (a1.x ^ b1.x) | (a1.y ^ b1.y) | (a1.z ^ b1.z) |
                     (a1.w ^ b1.w) | (a2.x ^ b2.x) | (a2.y ^ b2.y) | (a2.z ^ b2.z) | (a2.w ^ b2.w) | (a3.x ^ b3.x) | (a3.y ^ b3.y) |
                     (a3.z ^ b3.z);  // keys, versions, valid bytes, next, head (not the lock bytes)
  if (d != 0 || a3.y != KV_NULL || a3.z > KV_INLINE) return false;
  if (a3.z == KV_NULL || a3.x == 0) return true;  // (an empty bucket)
  uint64_t dv = 0;
#pragma unroll
  for (uint32_t s = 0; s < 4; s++)
    if ((a3.x >> (8 * s)) & 0xFFu) {
#pragma unroll
      for (uint32_t k = 0; k < VS / 8; k++)
        dv |= KV_LD(uint64_t, ea + KV_VAL_OFF + s * VS + 8 * k) ^ KV_LD(uint64_t, eb + KV_VAL_OFF + s * VS + 8 * k);
    }
  return dv == 0;
}
template <uint32_t VS>
__device__ static inline uint64_t ss_bucket_count(const kv_tab &ta, const kv_tab &tb, uint64_t b) {
  if (ss_bucket_equal_fast<VS>(ta, tb, b)) return 0;
  const ss_chain ca = {ta, b}, cb = {tb, b};
  ss_count_emit em;
  ss_bucket_diff(ca, cb, VS, SS_WALK_BOUND, em);
  return em.packed;
}

// cnt = this table's workgroup counts; stats = {only_a, only_b, val_differs, ver_only}
template <uint32_t VS>
__global__ void __launch_bounds__(SS_TB) k_state_diff_count(kv_tab ta, kv_tab tb, uint32_t *__restrict__ cnt, unsigned long long *stats) {
  __shared__ uint32_t red[SS_TB / 64][4];
  const uint64_t b = (uint64_t)blockIdx.x * SS_TB + threadIdx.x;
  const uint64_t packed = b < ta.n_local ? ss_bucket_count<VS>(ta, tb, b) : 0;
  sd_block_sum(red, {(uint32_t)packed & 0xFFFFu, (uint32_t)(packed >> 16) & 0xFFFFu, (uint32_t)(packed >> 32) & 0xFFFFu,
                     (uint32_t)(packed >> 48)});
  if (threadIdx.x < 4) {
    const uint32_t s = sd_block_total(red, threadIdx.x);
    if (s) atomicAdd(stats + threadIdx.x, (unsigned long long)s);
    red[0][threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) cnt[blockIdx.x] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
}

template <uint32_t VS>
__global__ void __launch_bounds__(SS_TB) k_state_diff_write(kv_tab ta, kv_tab tb, uint32_t table, const uint64_t *__restrict__ off,
                                                            uint8_t *out, uint64_t cap) {
  __shared__ uint32_t red[SS_TB / 64];
  const uint64_t at0 = off[blockIdx.x];
  if (at0 >= cap) return;  // (workgroup-uniform: everything this workgroup has lies behind the caller's buffer)
  const uint64_t b = (uint64_t)blockIdx.x * SS_TB + threadIdx.x;
  const uint64_t packed = b < ta.n_local ? ss_bucket_count<VS>(ta, tb, b) : 0;
  const uint32_t mine = (uint32_t)(packed & 0xFFFFu) + (uint32_t)((packed >> 16) & 0xFFFFu) + (uint32_t)((packed >> 32) & 0xFFFFu) +
                        (uint32_t)(packed >> 48);
  const uint32_t before = sd_block_excl_scan(red, mine);
  if (mine == 0 || at0 + before >= cap) return;
  const ss_chain ca = {ta, b}, cb = {tb, b};
  ss_write_emit<VS> em = {out, at0 + before, cap, table};
  ss_bucket_diff(ca, cb, VS, SS_WALK_BOUND, em);
}

// ------------------------------------------------------------------------------------------------------ repair
__device__ static inline uint64_t ss_rec_key(const uint8_t *r) { return *(const uint64_t *)r; }
// (table << 56 is never reached: a bucket index is below 2^32) -- the order the records must come in
__device__ static inline bool ss_rec_place(const kv_dev *kv, const uint8_t *r, uint64_t *place) {
  const uint32_t table = r[offsetof(LrRecord, table)];
  if (table >= kv->n_tables) return false;
  // (the LOCAL bucket: the global one on an unsharded engine; a record that is home to another shard has no place here)
  const uint64_t b = rr_local(ss_rec_key(r), table, kv->mod, kv->shard_index, kv->shard_count);
  if (b == SR_FOREIGN) return false;
  *place = ((uint64_t)table << 56) | b;
  return true;
}
// bad |= 1: a record that names a table the workload has not or is home to another shard (a log for dint_log_apply_device: any order)
__global__ void __launch_bounds__(SS_TB) k_state_home_check(const uint8_t *__restrict__ rec, uint64_t n, const kv_dev *__restrict__ kv,
                                                            uint32_t *bad) {
  const uint64_t i = (uint64_t)blockIdx.x * SS_TB + threadIdx.x;
  uint64_t me;
  if (i < n && !ss_rec_place(kv, rec + i * 64, &me)) atomicOr(bad, 1u);
}
__global__ void __launch_bounds__(SS_TB) k_state_repair_check(const uint8_t *__restrict__ rec, uint64_t n, const kv_dev *__restrict__ kv,
                                                              uint32_t *bad) {
  const uint64_t i = (uint64_t)blockIdx.x * SS_TB + threadIdx.x;
  if (i >= n) return;
  uint64_t me = 0, prev = 0;
  bool ok = ss_rec_place(kv, rec + i * 64, &me);
  if (ok && i > 0) ok = ss_rec_place(kv, rec + (i - 1) * 64, &prev) && prev <= me;
  if (!ok) atomicOr(bad, 1u);
}

// out = {updated, inserted, deleted, refused}; pend_off = the set of pend lists (in lists) an emptied entry is pushed to
__global__ void __launch_bounds__(SS_TB) k_state_repair(const uint8_t *__restrict__ rec, uint64_t n, const kv_dev *__restrict__ kv,
                                                        uint32_t pend_off, dint_dev_stats *stats, unsigned long long *out) {
  const uint64_t i0 = (uint64_t)blockIdx.x * SS_TB + threadIdx.x;
  uint32_t c[4] = {0, 0, 0, 0};
  uint64_t place = 0, prev = 0;
  bool head = i0 < n && ss_rec_place(kv, rec + i0 * 64, &place);
  if (head && i0 > 0 && ss_rec_place(kv, rec + (i0 - 1) * 64, &prev) && prev == place) head = false;  // inside another lane's run
  if (head) {
    const uint32_t table = (uint32_t)(place >> 56);
    const uint64_t bucket = place & 0x00FFFFFFFFFFFFFFull;
    kv_tab t = kv->tab[table];
    t.pend_head += pend_off;
    for (uint64_t i = i0; i < n; i++) {  // (at most the records of one bucket)
      const uint8_t *r = rec + i * 64;
      uint64_t pl;
      if (i > i0 && !(ss_rec_place(kv, r, &pl) && pl == place)) break;
      const uint64_t key = ss_rec_key(r);
      kv_hdr H;
      kv_hdr_load(H, kv_entry_ptr(t, bucket, KV_INLINE));
      if (r[offsetof(LrRecord, is_del)]) {
        if (kv_apply<ss_dev_mem>(t, bucket, H, KV_ACT_DEL, key, nullptr, 0, (uint32_t)bucket).ok) c[2]++;
        continue;
      }
      const uint32_t ver = *(const uint32_t *)(r + offsetof(LrRecord, ver));
      uint8_t *val = const_cast<uint8_t *>(r) + offsetof(LrRecord, val);
      const kv_where w = kv_locate(t, bucket, H, key);
      if (w.found) {  // the visible row takes the record's value AND version
        uint8_t *e = kv_entry_ptr(t, bucket, w.link);
        kv_copy_words(e + KV_VAL_OFF + w.slot * t.val_size, val, t.val_size);
        KV_ST(uint32_t, e + offsetof(kv_hdr, ver) + 4 * w.slot, ver);
        c[0]++;
      } else if (kv_apply<ss_dev_mem>(t, bucket, H, KV_ACT_INS, key, val, ver, (uint32_t)bucket).ok) {
        c[1]++;
      } else {
        c[3]++;
      }
    }
  }
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) {
    const uint32_t s = sd_wave_sum_u32(c[k]);
    if ((threadIdx.x & 63) == 0 && s) {
      atomicAdd(out + k, (unsigned long long)s);
      if (k == 3) atomicAdd(&stats->pool_exhausted, (unsigned long long)s);
    }
  }
}

// ------------------------------------------------------------------------------------------------------ host side
uint32_t dint_state_blocks(const dint_kv &kv) {
  uint64_t nb = 0;
  for (uint32_t t = 0; t < kv.n_tables; t++) nb += (kv.h.tab[t].n_local + SS_TB - 1) / SS_TB;
  return (uint32_t)nb;
}

void dint_launch_state_digest(const dint_kv &kv, dint_state_scratch s, hipStream_t st) {
  ss_digest_counts cnt = {{0, 0, 0, 0, 0}};
  for (uint32_t t = 0; t < kv.n_tables; t++) {
    const kv_tab &tb = kv.h.tab[t];
    const uint64_t tiles = ((tb.n_local + tb.pool_cap) * (tb.stride / 16) + SS_TILE_VEC - 1) / SS_TILE_VEC;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(tiles, SS_DIGEST_GRID));
    unsigned long long *part = s.digest_part + (size_t)4 * SS_DIGEST_GRID * t;
    cnt.n[t] = grid;
    if (tb.stride == 256) hipLaunchKernelGGL(k_state_digest<256>, dim3(grid), dim3(SS_TB), 0, st, tb, t, part);
    else hipLaunchKernelGGL(k_state_digest<128>, dim3(grid), dim3(SS_TB), 0, st, tb, t, part);
  }
  hipLaunchKernelGGL(k_state_digest_sum, dim3(kv.n_tables), dim3(SS_TB), 0, st, (const unsigned long long *)s.digest_part, cnt,
                     s.words + DINT_STATE_DIGEST_AT);
}

void dint_launch_state_diff_count(const dint_kv &a, const dint_kv &b, dint_state_scratch s, hipStream_t st) {
  (void)hipMemsetAsync(s.words, 0, 8 * sizeof(unsigned long long), st);
  const bool wide = a.val_size == 40;
  uint32_t at = 0;
  for (uint32_t t = 0; t < a.n_tables; t++) {
    const kv_tab &ta = a.h.tab[t], &tb = b.h.tab[t];
    const uint32_t nb = (uint32_t)((ta.n_local + SS_TB - 1) / SS_TB);
    if (wide) hipLaunchKernelGGL(k_state_diff_count<40>, dim3(nb), dim3(SS_TB), 0, st, ta, tb, s.blk_cnt + at, s.words);
    else hipLaunchKernelGGL(k_state_diff_count<8>, dim3(nb), dim3(SS_TB), 0, st, ta, tb, s.blk_cnt + at, s.words);
    at += nb;
  }
  sd_launch_scan((const uint32_t *)s.blk_cnt, at, s.blk_off, s.words + 4, st);
}

void dint_launch_state_diff_write(const dint_kv &a, const dint_kv &b, dint_state_scratch s, void *d_records, uint64_t cap, hipStream_t st) {
  const bool wide = a.val_size == 40;
  uint32_t at = 0;
  for (uint32_t t = 0; t < a.n_tables; t++) {
    const kv_tab &ta = a.h.tab[t], &tb = b.h.tab[t];
    const uint32_t nb = (uint32_t)((ta.n_local + SS_TB - 1) / SS_TB);
    if (wide) hipLaunchKernelGGL(k_state_diff_write<40>, dim3(nb), dim3(SS_TB), 0, st, ta, tb, t, (const uint64_t *)s.blk_off + at, (uint8_t *)d_records, cap);
    else hipLaunchKernelGGL(k_state_diff_write<8>, dim3(nb), dim3(SS_TB), 0, st, ta, tb, t, (const uint64_t *)s.blk_off + at, (uint8_t *)d_records, cap);
    at += nb;
  }
}

void dint_launch_state_repair_check(const dint_kv &kv, const void *d_records, uint64_t n, dint_state_scratch s, hipStream_t st) {
  (void)hipMemsetAsync(s.words + 8, 0, 8 * sizeof(unsigned long long), st);
  if (n == 0) return;
  hipLaunchKernelGGL(k_state_repair_check, dim3((uint32_t)((n + SS_TB - 1) / SS_TB)), dim3(SS_TB), 0, st, (const uint8_t *)d_records, n,
                     (const kv_dev *)kv.d_dev, (uint32_t *)(s.words + 8));
}

void dint_launch_state_home_check(const dint_kv &kv, const void *d_records, uint64_t n, dint_state_scratch s, hipStream_t st) {
  (void)hipMemsetAsync(s.words + DINT_STATE_HOME_AT, 0, sizeof(unsigned long long), st);
  if (n == 0) return;
  hipLaunchKernelGGL(k_state_home_check, dim3((uint32_t)((n + SS_TB - 1) / SS_TB)), dim3(SS_TB), 0, st, (const uint8_t *)d_records, n,
                     (const kv_dev *)kv.d_dev, (uint32_t *)(s.words + DINT_STATE_HOME_AT));
}

void dint_launch_state_repair(const dint_kv &kv, const void *d_records, uint64_t n, uint32_t pend_set, dint_dev_stats *stats,
                              dint_state_scratch s, hipStream_t st) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_state_repair, dim3((uint32_t)((n + SS_TB - 1) / SS_TB)), dim3(SS_TB), 0, st, (const uint8_t *)d_records, n,
                     (const kv_dev *)kv.d_dev, (pend_set & 1u) * KV_NLISTS, stats, s.words + 9);
}

// ---- the host forms (include/dint_driver.h): the same state_sync.h functions over dumped rows -------------------------
namespace {
inline uint64_t host_row_hash(uint64_t key, uint32_t ver, uint32_t table, const uint8_t *val, uint32_t val_size) {
  return ss_row_hash(key, ver, table, val_size, [val](uint32_t k) { return si_ld64(val + 8 * k); });
}
// the rows of one bucket out of a dump: idx[lo .. hi) index the dumped arrays, in dump (= chain) order
struct host_rows {
  const uint64_t *keys;
  const uint32_t *vers;
  const uint8_t *vals;
  uint32_t val_size;
  const uint64_t *idx;
  uint64_t n;
  uint64_t begin() const { return 0; }
  uint64_t next(uint64_t p) const { return p + 1; }
  bool ok(uint64_t p) const { return p < n; }
  bool same(uint64_t p, uint64_t q) const { return p == q; }
  uint64_t key(uint64_t p) const { return keys[idx[p]]; }
  uint32_t ver(uint64_t p) const { return vers[idx[p]]; }
  uint32_t val32(uint64_t p, uint32_t w) const { return si_ld32(vals + idx[p] * val_size + 4 * w); }
  uint64_t find(uint64_t k) const {
    for (uint64_t p = 0; p < n; p++)
      if (keys[idx[p]] == k) return p;
    return n;
  }
};
struct host_emit {
  uint8_t *out;
  uint64_t at, cap;
  uint32_t table, val_size;
  uint64_t kinds[4];
  void operator()(uint32_t kind, const host_rows &l, uint64_t p) {
    kinds[kind]++;
    if (at < cap) {
      uint32_t w[16];
      ss_fill_record(w, kind, l, p, table, val_size);
      memcpy(out + at * 64, w, 64);
    }
    at++;
  }
};
}  // namespace

extern "C" uint64_t dint_state_row_hash_host(uint64_t key, uint32_t ver, uint32_t table, const void *val, uint32_t val_size) {
  if (!val || (val_size != 40 && val_size != 8)) return 0;
  return host_row_hash(key, ver, table, (const uint8_t *)val, val_size);
}

extern "C" int dint_state_digest_host(uint32_t table, const uint64_t *keys, const uint32_t *vers, const void *vals, uint32_t val_size,
                                      uint64_t n, dint_table_digest *out) {
  if (!out || (n && (!keys || !vers || !vals)) || (val_size != 40 && val_size != 8)) return DINT_EINVAL;
  ss_digest d = {0, 0, 0};
  for (uint64_t i = 0; i < n; i++) ss_digest_add(d, host_row_hash(keys[i], vers[i], table, (const uint8_t *)vals + i * val_size, val_size));
  out->rows = d.rows; out->sum = d.sum; out->xr = d.xr; out->reserved = 0;
  return 0;
}

extern "C" int64_t dint_state_diff_host(uint32_t table, uint64_t hash_size, uint32_t val_size, const uint64_t *a_keys,
                                        const uint32_t *a_vers, const void *a_vals, uint64_t na, const uint64_t *b_keys,
                                        const uint32_t *b_vers, const void *b_vals, uint64_t nb, void *records, uint64_t cap,
                                        dint_diff_stats *out) {
  if (hash_size == 0 || (val_size != 40 && val_size != 8) || table > 255 || (na && (!a_keys || !a_vers || !a_vals)) ||
      (nb && (!b_keys || !b_vers || !b_vals)) || (cap && !records))
    return DINT_EINVAL;
  try {
    // rows grouped by bucket, dump order kept inside a bucket (a stable sort), then the two lists walked bucket by bucket
    const dint_mod mod = dint_make_mod(hash_size);
    auto group = [&](const uint64_t *keys, uint64_t n, std::vector<uint64_t> &bkt, std::vector<uint64_t> &idx) {
      bkt.resize(n);
      idx.resize(n);
      for (uint64_t i = 0; i < n; i++) bkt[i] = dint_fastmod(dint_hash_key(keys[i]), mod);
      std::iota(idx.begin(), idx.end(), 0ull);
      std::stable_sort(idx.begin(), idx.end(), [&](uint64_t x, uint64_t y) { return bkt[x] < bkt[y]; });
    };
    std::vector<uint64_t> ba, ia, bb, ib;
    group(a_keys, na, ba, ia);
    group(b_keys, nb, bb, ib);
    host_emit em = {(uint8_t *)records, 0, cap, table, val_size, {0, 0, 0, 0}};
    uint64_t pa = 0, pb = 0;
    while (pa < na || pb < nb) {
      const uint64_t bucket = std::min(pa < na ? ba[ia[pa]] : ~0ull, pb < nb ? bb[ib[pb]] : ~0ull);
      uint64_t ea = pa, eb = pb;
      while (ea < na && ba[ia[ea]] == bucket) ea++;
      while (eb < nb && bb[ib[eb]] == bucket) eb++;
      const host_rows la = {a_keys, a_vers, (const uint8_t *)a_vals, val_size, ia.data() + pa, ea - pa};
      const host_rows lb = {b_keys, b_vers, (const uint8_t *)b_vals, val_size, ib.data() + pb, eb - pb};
      ss_bucket_diff(la, lb, val_size, 0xFFFFFFFFu, em);
      pa = ea;
      pb = eb;
    }
    if (out) {
      memset(out, 0, sizeof *out);
      out->total = em.at;
      out->only_a = em.kinds[SS_ONLY_A]; out->only_b = em.kinds[SS_ONLY_B];
      out->val_differs = em.kinds[SS_VAL]; out->ver_only = em.kinds[SS_VER];
    }
    return (int64_t)std::min(em.at, cap);
  } catch (const std::bad_alloc &) {
    return DINT_ENOMEM;
  }
}
