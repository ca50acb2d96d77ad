// state_dev.h -- device-side building blocks of the state kernels, the units that read a server's tables where they lie:
// k_state.hip (digest / diff / repair), k_block.hip (the same block by block), k_image.hip (export / import), k_rehash.hip,
// k_stats.hip (the table report) and k_verify.hip (the census of chains, lists and pool).  None
// of it is on a request's path, and no other unit includes it.  wave_excl_scan_u32 is dint_device.h's; the rules that host and
// device share (the chain walk among them) are state_image.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dint_device.h"
#include "dint_kv_core.h"
#include "state_image.h"
#include "state_sync.h"

#define SD_TB 256u  // threads per workgroup of every kernel that uses the workgroup helpers below

typedef uint32_t sd_v4 __attribute__((ext_vector_type(4)));  // a 16-byte vector the compiler knows (address spaces, non-temporal loads)
typedef uint32_t sd_v2 __attribute__((ext_vector_type(2)));

// ---- the wave ----------------------------------------------------------------------------------------------------------
__device__ static inline uint64_t sd_shfl_xor_u64(uint64_t v, int d) {
  const uint32_t lo = __shfl_xor((uint32_t)v, d, 64), hi = __shfl_xor((uint32_t)(v >> 32), d, 64);
  return ((uint64_t)hi << 32) | lo;
}
__device__ static inline uint32_t sd_wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ static inline uint32_t sd_wave_max_u32(uint32_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = max(v, (uint32_t)__shfl_xor(v, d, 64));
  return v;
}
__device__ static inline uint64_t sd_wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += sd_shfl_xor_u64(v, d);
  return v;
}
__device__ static inline uint64_t sd_wave_xor_u64(uint64_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v ^= sd_shfl_xor_u64(v, d);
  return v;
}

// q = h / f.d (dint_device.h dint_fastmod's quotient)
__device__ static inline uint64_t sd_div(uint64_t h, dint_mod f) {
  if (f.d <= 1) return h;
  uint64_t q = __umul64hi(h, f.m);
  if (h - q * f.d >= f.d) q++;
  return q;
}

// ---- the workgroup (SD_TB threads; every thread calls, before any of them returns) -----------------------------------------------
// K per-lane numbers to K per-workgroup totals: the wave reduction, one LDS word per wave and number, one barrier.  Afterwards
// sd_block_total(red, k) is number k's total in whichever thread asks (thread 0 for all of them, or thread k for its own).
template <uint32_t K>
__device__ static inline void sd_block_sum(uint32_t (&red)[SD_TB / 64][K], const uint32_t (&v)[K]) {
  uint32_t s[K];
#pragma unroll
  for (uint32_t k = 0; k < K; k++) s[k] = sd_wave_sum_u32(v[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (uint32_t k = 0; k < K; k++) red[threadIdx.x >> 6][k] = s[k];
  }
  __syncthreads();
}
template <uint32_t K>
__device__ static inline uint32_t sd_block_total(const uint32_t (&red)[SD_TB / 64][K], uint32_t k) {
  uint32_t s = 0;
  for (uint32_t w = 0; w < SD_TB / 64; w++) s += red[w][k];
  return s;
}
// the sum of `v` over the threads below this one
__device__ static inline uint32_t sd_block_excl_scan(uint32_t (&red)[SD_TB / 64], uint32_t v) {
  uint32_t tot;
  uint32_t before = wave_excl_scan_u32(v, &tot);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = tot;
  __syncthreads();
  for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) before += red[w];
  return before;
}

// ---- the scan of the workgroups' counts --------------------------------------------------------------------------------------
// T = uint32_t: off[i] = cnt[0] + .. + cnt[i - 1], total[0] = the sum.  T = sd_v2 {x, y}: the same over the .x, and total[1] = the
// sum of the .y.  One workgroup of 1,024; a thread owns (nb + 1023) / 1024 consecutive counts.
__device__ static inline uint32_t sd_scan_x(uint32_t c) { return c; }
__device__ static inline uint32_t sd_scan_x(sd_v2 c) { return c.x; }
__device__ static inline uint32_t sd_scan_y(uint32_t) { return 0; }
__device__ static inline uint32_t sd_scan_y(sd_v2 c) { return c.y; }
template <class T>
__global__ void __launch_bounds__(1024) k_state_scan(const T *__restrict__ cnt, uint32_t nb, uint64_t *__restrict__ off,
                                                     unsigned long long *total) {
  constexpr bool PAIR = sizeof(T) == sizeof(sd_v2);
  __shared__ uint64_t part[PAIR ? 2 : 1][1024];  // [0] the .x, [1] the .y
  const uint32_t t = threadIdx.x, per = (nb + 1023u) / 1024u;
  const uint32_t lo = min(nb, t * per), hi = min(nb, lo + per);
  uint64_t s = 0, sy = 0;
  for (uint32_t i = lo; i < hi; i++) {
    const T c = cnt[i];
    s += sd_scan_x(c);
    sy += sd_scan_y(c);
  }
  part[0][t] = s;
  if (PAIR) part[PAIR][t] = sy;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {  // inclusive scan of the threads' sums
    const uint64_t y = t >= d ? part[0][t - d] : 0, yy = PAIR && t >= d ? part[PAIR][t - d] : 0;
    __syncthreads();
    part[0][t] += y;
    if (PAIR) part[PAIR][t] += yy;
    __syncthreads();
  }
  uint64_t run = part[0][t] - s;
  for (uint32_t i = lo; i < hi; i++) {
    off[i] = run;
    run += sd_scan_x(cnt[i]);
  }
  if (t == 1023) {
    total[0] = part[0][1023];
    if (PAIR) total[1] = part[PAIR][1023];
  }
}
template <class T>
static inline void sd_launch_scan(const T *cnt, uint32_t nb, uint64_t *off, unsigned long long *total, hipStream_t st) {
  hipLaunchKernelGGL(k_state_scan<T>, dim3(1), dim3(1024), 0, st, cnt, nb, off, total);
}

// ---- one bucket of a table as it lies in HBM ---------------------------------------------------------------------------------
// local bucket b of table t; lv = the 16-byte link vector {validw, next, head, lockw} of its inline header, loaded once: the
// inline entry's links are answered from it, an overflow entry's from 8 bytes of its header.  The accessor of state_image.h
// si_chain_walk and of state_stats.h st_bucket_walk.
struct sd_bucket {
  const kv_tab &t;
  uint64_t b;
  sd_v4 lv;
  __device__ inline uint32_t head() const { return lv.z; }
  __device__ inline bool link_ok(uint32_t link) const { return link - 2u < t.pool_cap; }
  __device__ inline void links(uint32_t link, uint32_t &validw, uint32_t &next) const {
    if (link == KV_INLINE) {
      validw = lv.x;
      next = lv.y;
    } else {
      const sd_v2 v = *(const KV_G(sd_v2) *)(kv_entry_ptr(t, b, link) + KV_VALID_OFF);
      validw = v.x;
      next = v.y;
    }
  }
  __device__ inline void keys(uint32_t link, uint64_t k[4]) const {
    const KV_G(sd_v4) *p = (const KV_G(sd_v4) *)kv_entry_ptr(t, b, link);
    const sd_v4 a = p[0], c = p[1];
    k[0] = (uint64_t)a.x | ((uint64_t)a.y << 32);
    k[1] = (uint64_t)a.z | ((uint64_t)a.w << 32);
    k[2] = (uint64_t)c.x | ((uint64_t)c.y << 32);
    k[3] = (uint64_t)c.z | ((uint64_t)c.w << 32);
  }
  // the eight smallbank counter words of the inline header (state_image.h si_locks_held)
  __device__ inline void sb_counters(uint32_t c[8]) const {
    const KV_G(sd_v4) *p = (const KV_G(sd_v4) *)(kv_entry_ptr(t, b, KV_INLINE) + KV_SB_LOCK_OFF);
    const sd_v4 c0 = p[0], c1 = p[1];
    c[0] = c0.x; c[1] = c0.y; c[2] = c0.z; c[3] = c0.w;
    c[4] = c1.x; c[5] = c1.y; c[6] = c1.z; c[7] = c1.w;
  }
  __device__ inline uint32_t locks_held(uint32_t lock_mode) const {
    return si_locks_held(lock_mode, lv.w, [this](uint32_t c[8]) { sb_counters(c); });
  }
};
__device__ static inline sd_bucket sd_bucket_at(const kv_tab &t, uint64_t b) {
  return sd_bucket{t, b, *((const KV_G(sd_v4) *)kv_entry_ptr(t, b, KV_INLINE) + SI_LINK_VEC)};
}
// state_image.h si_walk_chain over the bucket; head 0, or head 1 with no successor -> no walk (most buckets of most tables)
template <class F>
__device__ static inline si_walk sd_bucket_walk(const sd_bucket &ch, F &&on_ovf) {
  if (ch.lv.z == KV_NULL) return si_walk{0, 0, 0, 0, 1};
  if (ch.lv.z == KV_INLINE && ch.lv.y == KV_NULL) return si_walk{0, 0, si_valid_count(ch.lv.x), 1, 1};
  return si_walk_chain(ch.lv.z, ch, on_ovf);
}

// ---- the digest of a workgroup ------------------------------------------------------------------------------------------------
// the workgroup's digest of the lanes' d, in thread 0 (every thread calls: the wave, one LDS word per wave and number, one barrier)
__device__ static inline ss_digest ss_block_digest(uint64_t (&red)[SD_TB / 64][3], ss_digest d) {
  d.rows = sd_wave_sum_u64(d.rows);
  d.sum = sd_wave_sum_u64(d.sum);
  d.xr = sd_wave_xor_u64(d.xr);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = d.rows; red[threadIdx.x >> 6][1] = d.sum; red[threadIdx.x >> 6][2] = d.xr; }
  __syncthreads();
  ss_digest w = {0, 0, 0};
  if (threadIdx.x == 0)
    for (uint32_t k = 0; k < SD_TB / 64; k++) ss_digest_merge(w, ss_digest{red[k][0], red[k][1], red[k][2]});
  return w;
}

// ---- a bucket's rows for state_sync.h ss_bucket_diff (k_state.hip the diff, k_block.hip the block rows and the block diff) ----------
// the rows of one bucket in chain order, read from the table as it lies in HBM.  A position is link << 2 | slot; 0 = the end.
struct ss_chain {
  kv_tab t;
  uint64_t b;
  __device__ inline bool link_ok(uint32_t link) const { return link == KV_INLINE || (link >= 2u && link - 2u < t.pool_cap); }
  __device__ inline const uint8_t *entry(uint64_t p) const { return kv_entry_ptr(t, b, (uint32_t)(p >> 2)); }
  // the first valid slot at or behind (link, slot)
  __device__ inline uint64_t seek(uint32_t link, uint32_t slot) const {
    for (uint32_t steps = 0; link_ok(link) && steps < KV_MAX_CHAIN; steps++) {
      const uint8_t *e = kv_entry_ptr(t, b, link);
      const uint32_t vw = KV_LD(uint32_t, e + KV_VALID_OFF);
      for (; slot < 4; slot++)
        if ((vw >> (8 * slot)) & 0xFFu) return ((uint64_t)link << 2) | slot;
      link = KV_LD(uint32_t, e + offsetof(kv_hdr, next));
      slot = 0;
    }
    return 0;
  }
  __device__ inline uint64_t begin() const { return seek(KV_LD(uint32_t, kv_entry_ptr(t, b, KV_INLINE) + offsetof(kv_hdr, head)), 0); }
  __device__ inline uint64_t next(uint64_t p) const { return seek((uint32_t)(p >> 2), (uint32_t)(p & 3) + 1); }
  __device__ inline bool ok(uint64_t p) const { return p != 0; }
  __device__ inline bool same(uint64_t p, uint64_t q) const { return p == q; }
  __device__ inline uint64_t key(uint64_t p) const { return KV_LD(uint64_t, entry(p) + 8 * (p & 3)); }
  __device__ inline uint32_t ver(uint64_t p) const { return KV_LD(uint32_t, entry(p) + 32 + 4 * (p & 3)); }
  __device__ inline uint32_t val32(uint64_t p, uint32_t w) const {
    return KV_LD(uint32_t, entry(p) + KV_VAL_OFF + (p & 3) * t.val_size + 4 * w);
  }
  __device__ inline uint64_t find(uint64_t k) const {
    uint32_t link = KV_LD(uint32_t, kv_entry_ptr(t, b, KV_INLINE) + offsetof(kv_hdr, head));
    for (uint32_t steps = 0; link_ok(link) && steps < KV_MAX_CHAIN; steps++) {
      kv_hdr h;
      kv_hdr_load(h, kv_entry_ptr(t, b, link));
#pragma unroll
      for (uint32_t i = 0; i < 4; i++)
        if (kv_valid(h, i) && h.key[i] == k) return ((uint64_t)link << 2) | i;
      link = h.next;
    }
    return 0;
  }
};
#define SS_WALK_BOUND (4u * KV_MAX_CHAIN)  // rows a bucket's walk visits at most: the counts below fit 16 bits each

struct ss_count_emit {
  uint64_t packed = 0;  // four 16-bit counts, kind k in bits 16k..
  template <class L, class P>
  __device__ inline void operator()(uint32_t kind, const L &, P) { packed += 1ull << (16 * kind); }
};
template <uint32_t VS>
struct ss_write_emit {
  uint8_t *out;
  uint64_t at, cap;
  uint32_t table;
  template <class L, class P>
  __device__ inline void operator()(uint32_t kind, const L &l, P p) {
    if (at < cap) {
      uint32_t w[16];
      ss_fill_record(w, kind, l, p, table, VS);
      uint64_t *o = (uint64_t *)(out + at * 64);
#pragma unroll
      for (uint32_t k = 0; k < 8; k++) o[k] = (uint64_t)w[2 * k] | ((uint64_t)w[2 * k + 1] << 32);
    }
    at++;
  }
};
