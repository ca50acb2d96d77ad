// k_image.hip -- an engine's tables written out as a position-independent image and read back into another shard layout
// without leaving the GPU (include/dint_abi.h dint_state_export / dint_state_import, driven by engine.hip; the format and
// the per-entry rules live in state_image.h, which the host form at the end of this file shares).
//
//   k_image_count      one lane per SELECTED bucket (local bucket l0 + k * step of the source: state_image.h si_select): the
//                      overflow entries and valid slots of its chain.  Reads the 16-byte link vector of the inline header;
//                      head 0, or head 1 with no successor -> no walk.  Per workgroup one {entries, slots} pair.
//   k_state_scan       (state_dev.h) exclusive scan of the workgroups' entry counts of one table, and the two totals
//   k_image_dir        (the host has read the totals and knows the image's size by now)  the count again, a scan inside the
//                      workgroup: the bucket's directory record {global bucket, first, count} goes to the image, its two
//                      rewritten link words and -- buckets with overflow entries walk a second time -- the pool index of
//                      every overflow entry in chain order go to scratch
//   k_image_copy_out   the stream: inline entries, then overflow entries, as 16-byte vectors (16 lanes per 256-byte entry, 8
//                      per 128-byte entry, SI_UNROLL entries per lane, all loads before the first store); the lane that holds
//                      the link vector patches it
//   k_image_check      one lane per bucket of an IMAGE: state_image.h si_check_bucket / si_check_slot.  Runs before import
//                      touches a table; import follows no link, so a bad image costs a refusal and nothing else.
//   k_image_copy_in    the stream back: bucket g to local bucket g / H, overflow entry x to pool entry base + x, links >= 2
//                      moved by base; one workgroup's first lane sets pool_top.  No atomics: every entry has one lane group.
//   k_image_lock_out / k_image_lock_in   lock tables: {global slot, a, b} per selected slot
// Every chain walk is state_image.h si_chain_walk: to KV_MAX_CHAIN entries, every link checked against the pool's size (export:
// state_dev.h sd_bucket) or the bucket's run (check: si_image_chain) before it is followed.
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

#define SI_TB SD_TB    // threads per workgroup, every kernel here
#define SI_UNROLL 4u   // copy kernels: entries per lane group (vectors in flight per lane)

// ------------------------------------------------------------------------------------------------------ export
// blk[workgroup] = {overflow entries, valid slots} of its 256 selected buckets; *badw |= 1: a chain that does not end, or has
// more overflow entries than the check accepts (SI_MAX_RUN): an engine never exports an image its own import refuses
__global__ void __launch_bounds__(SI_TB) k_image_count(kv_tab t, si_sel s, sd_v2 *__restrict__ blk, uint32_t *badw) {
  __shared__ uint32_t red[SI_TB / 64][2];
  const uint64_t k = (uint64_t)blockIdx.x * SI_TB + threadIdx.x;
  uint32_t c = 0, r = 0;
  if (k < s.n) {
    const si_walk w = sd_bucket_walk(sd_bucket_at(t, s.l0 + k * s.step), [](uint32_t, uint32_t) { return true; });
    c = w.count;
    r = w.rows;
    if (!w.ok || w.count > SI_MAX_RUN) atomicOr(badw, 1u);
  }
  sd_block_sum(red, {c, r});
  if (threadIdx.x == 0) blk[blockIdx.x] = sd_v2{sd_block_total(red, 0), sd_block_total(red, 1)};
}

// dir[k] = bucket k's directory record; inl[k] = {head, next} of its inline entry as the image has them; ovf_src[x] = the pool
// index of what becomes overflow entry x (n_ovf of them: nothing is stored beyond, whatever the tables say by now)
__global__ void __launch_bounds__(SI_TB) k_image_dir(kv_tab t, si_sel s, const uint64_t *__restrict__ blk_off, sd_v4 *__restrict__ dir,
                                                     sd_v2 *__restrict__ inl, uint32_t *__restrict__ ovf_src, uint64_t n_ovf) {
  __shared__ uint32_t red[SI_TB / 64];
  const uint64_t k = (uint64_t)blockIdx.x * SI_TB + threadIdx.x;
  const uint64_t b = s.l0 + k * s.step;
  sd_v4 lv = {0, 0, 0, 0};
  si_walk w = {0, 0, 0, 0, 1};
  if (k < s.n) {
    const sd_bucket ch = sd_bucket_at(t, b);
    lv = ch.lv;
    w = sd_bucket_walk(ch, [](uint32_t, uint32_t) { return true; });
  }
  const uint32_t before = sd_block_excl_scan(red, w.count);
  if (k >= s.n) return;
  const uint64_t first = blk_off[blockIdx.x] + before, g = b * s.G + s.i;
  dir[k] = sd_v4{(uint32_t)g, (uint32_t)(g >> 32), (uint32_t)first, w.count};
  inl[k] = sd_v2{si_head_out(lv.z, first), si_inline_next_out(lv.y, w.linked != 0, first, w.before)};
  if (w.count)
    sd_bucket_walk(sd_bucket_at(t, b), [=](uint32_t m, uint32_t link) {
      if (first + m < n_ovf) ovf_src[first + m] = link - 2u;
      return true;
    });
}

// entries [0, s.n) = the selected inline entries, [s.n, s.n + n_ovf) = the overflow entries in image order
template <uint32_t STRIDE>
__global__ void __launch_bounds__(SI_TB) k_image_copy_out(kv_tab t, si_sel s, uint64_t n_ovf, const sd_v2 *__restrict__ inl,
                                                          const uint32_t *__restrict__ ovf_src, uint8_t *img_inl, uint8_t *img_ovf) {
  constexpr uint32_t VPE = STRIDE / 16, EPS = SI_TB / VPE;  // vectors per entry, entries per step of the workgroup
  const uint32_t v = threadIdx.x % VPE;
  const uint64_t e0 = (uint64_t)blockIdx.x * (EPS * SI_UNROLL) + threadIdx.x / VPE, n = s.n + n_ovf;
  sd_v4 x[SI_UNROLL];
  sd_v2 l[SI_UNROLL];
#pragma unroll
  for (uint32_t u = 0; u < SI_UNROLL; u++) {
    const uint64_t e = e0 + u * EPS;
    if (e >= n) continue;
    uint64_t at;
    if (e < s.n) {
      at = s.l0 + e * s.step;
      if (v == SI_LINK_VEC) l[u] = inl[e];
    } else {
      const uint32_t p = ovf_src[e - s.n];
      at = t.n_local + (p < t.pool_cap ? p : 0u);
    }
    x[u] = __builtin_nontemporal_load((const KV_G(sd_v4) *)(t.entries + at * STRIDE) + v);
  }
#pragma unroll
  for (uint32_t u = 0; u < SI_UNROLL; u++) {
    const uint64_t e = e0 + u * EPS;
    if (e >= n) continue;
    if (v == SI_LINK_VEC) {
      if (e < s.n) { x[u].z = l[u].x; x[u].y = l[u].y; }
      else x[u].y = si_next_out(x[u].y, e - s.n);
    }
    uint8_t *dst = e < s.n ? img_inl + e * STRIDE : img_ovf + (e - s.n) * STRIDE;
    __builtin_nontemporal_store(x[u], (KV_G(sd_v4) *)dst + v);
  }
}

// lock tables: out == nullptr only counts.  blk[workgroup] = {0, slots with a non-zero word}
__global__ void __launch_bounds__(SI_TB) k_image_lock_out(const uint2 *__restrict__ tbl, si_sel s, sd_v4 *__restrict__ out,
                                                          sd_v2 *__restrict__ blk) {
  __shared__ uint32_t red[SI_TB / 64][1];
  const uint64_t k = (uint64_t)blockIdx.x * SI_TB + threadIdx.x;
  uint32_t r = 0;
  if (k < s.n) {
    const uint64_t l = s.l0 + k * s.step, g = l * s.G + s.i;
    const sd_v2 w = *((const KV_G(sd_v2) *)tbl + l);
    r = (w.x | w.y) != 0;
    if (out) out[k] = sd_v4{(uint32_t)g, (uint32_t)(g >> 32), w.x, w.y};
  }
  sd_block_sum(red, {r});
  if (threadIdx.x == 0) blk[blockIdx.x] = sd_v2{0, sd_block_total(red, 0)};
}

// ------------------------------------------------------------------------------------------------------ import
// one table's section of an image in device memory
struct si_dev_image {
  const uint8_t *p_dir, *p_inl, *p_ovf;
  uint32_t stride;
  __device__ inline si_dir dir(uint64_t b) const {
    const sd_v4 v = *((const KV_G(sd_v4) *)p_dir + b);
    return si_dir{(uint64_t)v.x | ((uint64_t)v.y << 32), v.z, v.w};
  }
  __device__ inline void inline_links(uint64_t b, uint32_t &validw, uint32_t &next, uint32_t &head) const {
    const sd_v4 v = *((const KV_G(sd_v4) *)(p_inl + b * stride) + SI_LINK_VEC);
    validw = v.x; next = v.y; head = v.z;
  }
  __device__ inline void ovf_links(uint64_t x, uint32_t &validw, uint32_t &next) const {
    const sd_v2 v = *(const KV_G(sd_v2) *)(p_ovf + x * stride + KV_VALID_OFF);
    validw = v.x; next = v.y;
  }
};

// *badw |= what the check found; blk[workgroup] = {0, valid slots}
__global__ void __launch_bounds__(SI_TB) k_image_check(si_dev_image im, si_geom g, int lock, uint32_t *badw, sd_v2 *__restrict__ blk) {
  __shared__ uint32_t red[SI_TB / 64][1];
  const uint64_t b = (uint64_t)blockIdx.x * SI_TB + threadIdx.x;
  uint32_t bad = 0, r = 0;
  if (b < g.n_buckets) {
    if (lock) {
      bad = si_check_slot(im, b, g);
      const si_dir d = im.dir(b);
      r = (d.first | d.count) != 0;
    } else {
      uint64_t rows = 0;
      bad = si_check_bucket(im, b, g, &rows);
      r = (uint32_t)rows;
    }
  }
  if (bad) atomicOr(badw, bad);
  sd_block_sum(red, {r});
  if (threadIdx.x == 0) blk[blockIdx.x] = sd_v2{0, sd_block_total(red, 0)};
}

// the checked image into the table: bucket id to local bucket id / H, overflow entry x to pool entry base + x
template <uint32_t STRIDE>
__global__ void __launch_bounds__(SI_TB) k_image_copy_in(kv_tab t, dint_mod H, uint64_t n_b, uint64_t n_ovf, uint32_t base, si_dev_image im) {
  constexpr uint32_t VPE = STRIDE / 16, EPS = SI_TB / VPE;
  const uint32_t v = threadIdx.x % VPE;
  const uint64_t e0 = (uint64_t)blockIdx.x * (EPS * SI_UNROLL) + threadIdx.x / VPE, n = n_b + n_ovf;
  sd_v4 x[SI_UNROLL];
  uint64_t at[SI_UNROLL];
#pragma unroll
  for (uint32_t u = 0; u < SI_UNROLL; u++) {
    const uint64_t e = e0 + u * EPS;
    at[u] = ~0ull;
    if (e >= n) continue;
    const uint8_t *src;
    if (e < n_b) {
      const uint64_t local = sd_div(*((const KV_G(uint64_t) *)(im.p_dir + 16 * e)), H);
      if (local < t.n_local) at[u] = local;
      src = im.p_inl + e * STRIDE;
    } else {
      const uint64_t p = (uint64_t)base + (e - n_b);
      if (p < t.pool_cap) at[u] = t.n_local + p;
      src = im.p_ovf + (e - n_b) * STRIDE;
    }
    x[u] = __builtin_nontemporal_load((const KV_G(sd_v4) *)src + v);
  }
#pragma unroll
  for (uint32_t u = 0; u < SI_UNROLL; u++) {
    if (at[u] == ~0ull) continue;
    if (v == SI_LINK_VEC) {
      x[u].y = si_link_in(x[u].y, base);
      if (e0 + u * EPS < n_b) x[u].z = si_link_in(x[u].z, base);
    }
    *((KV_G(sd_v4) *)(t.entries + at[u] * STRIDE) + v) = x[u];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) KV_ST(uint32_t, t.pool_top, base + (uint32_t)n_ovf);
}

__global__ void __launch_bounds__(SI_TB) k_image_lock_in(uint2 *__restrict__ tbl, uint64_t n_local, dint_mod H, uint64_t n, si_dev_image im) {
  const uint64_t k = (uint64_t)blockIdx.x * SI_TB + threadIdx.x;
  if (k >= n) return;
  const si_dir d = im.dir(k);
  const uint64_t local = sd_div(d.id, H);
  if (local < n_local) *((KV_G(sd_v2) *)tbl + local) = sd_v2{d.first, d.count};
}

// ------------------------------------------------------------------------------------------------------ host side
static inline uint32_t si_blocks(uint64_t n) { return (uint32_t)((n + SI_TB - 1) / SI_TB); }
static inline uint32_t si_copy_blocks(uint64_t entries, uint32_t stride) {
  const uint64_t per = (uint64_t)(SI_TB / (stride / 16)) * SI_UNROLL;
  return (uint32_t)((entries + per - 1) / per);
}

uint32_t dint_image_blocks(const uint64_t *n, uint32_t n_tables) {
  uint64_t nb = 0;
  for (uint32_t t = 0; t < n_tables; t++) nb += si_blocks(n[t]);
  return (uint32_t)nb;
}

void dint_launch_image_count(const dint_kv &kv, const si_sel *sel, dint_image_scratch s, hipStream_t st) {
  (void)hipMemsetAsync(s.words, 0, DINT_IMAGE_WORDS * sizeof(unsigned long long), st);
  uint32_t at = 0;
  for (uint32_t t = 0; t < kv.n_tables; t++) {
    const uint32_t nb = si_blocks(sel[t].n);
    if (nb) {
      hipLaunchKernelGGL(k_image_count, dim3(nb), dim3(SI_TB), 0, st, kv.h.tab[t], sel[t], (sd_v2 *)s.blk + at, (uint32_t *)(s.words + DINT_IMAGE_BAD_AT));
      sd_launch_scan((const sd_v2 *)s.blk + at, nb, s.blk_off + at, s.words + 2 * t, st);
    }
    at += nb;
  }
}

void dint_launch_image_write(const dint_kv &kv, const si_sel *sel, const si_header &h, dint_image_scratch s, uint8_t *d_buf, hipStream_t st) {
  uint32_t at = 0;
  uint64_t inl_at = 0, ovf_at = 0;
  for (uint32_t t = 0; t < kv.n_tables; t++) {
    const kv_tab &tb = kv.h.tab[t];
    const si_table &it = h.table[t];
    const uint32_t nb = si_blocks(sel[t].n);
    if (nb) {
      uint8_t *dir = d_buf + it.offset, *img_inl = dir + 16 * it.n_buckets, *img_ovf = img_inl + it.n_buckets * tb.stride;
      sd_v2 *inl = (sd_v2 *)s.inl + inl_at;
      uint32_t *ovf_src = s.ovf_src + ovf_at;
      hipLaunchKernelGGL(k_image_dir, dim3(nb), dim3(SI_TB), 0, st, tb, sel[t], (const uint64_t *)s.blk_off + at, (sd_v4 *)dir, inl, ovf_src,
                         it.n_overflow);
      const uint32_t cb = si_copy_blocks(it.n_buckets + it.n_overflow, tb.stride);
      if (tb.stride == 256)
        hipLaunchKernelGGL(k_image_copy_out<256>, dim3(cb), dim3(SI_TB), 0, st, tb, sel[t], it.n_overflow, (const sd_v2 *)inl,
                           (const uint32_t *)ovf_src, img_inl, img_ovf);
      else
        hipLaunchKernelGGL(k_image_copy_out<128>, dim3(cb), dim3(SI_TB), 0, st, tb, sel[t], it.n_overflow, (const sd_v2 *)inl,
                           (const uint32_t *)ovf_src, img_inl, img_ovf);
    }
    at += nb;
    inl_at += it.n_buckets;
    ovf_at += it.n_overflow;
  }
}

void dint_launch_image_lock_out(const uint2 *tbl, si_sel sel, uint8_t *d_slots, dint_image_scratch s, hipStream_t st) {
  (void)hipMemsetAsync(s.words, 0, DINT_IMAGE_WORDS * sizeof(unsigned long long), st);
  const uint32_t nb = si_blocks(sel.n);
  if (!nb) return;
  hipLaunchKernelGGL(k_image_lock_out, dim3(nb), dim3(SI_TB), 0, st, tbl, sel, (sd_v4 *)d_slots, (sd_v2 *)s.blk);
  sd_launch_scan((const sd_v2 *)s.blk, nb, s.blk_off, s.words, st);
}

static si_dev_image si_section(const si_header &h, uint32_t t, const uint8_t *d_buf, bool lock) {
  const si_table &it = h.table[t];
  si_dev_image im;
  im.p_dir = d_buf + it.offset;
  im.p_inl = im.p_dir + 16 * it.n_buckets;
  im.p_ovf = lock ? im.p_inl : im.p_inl + it.n_buckets * h.stride;
  im.stride = h.stride;
  return im;
}
static si_geom si_geometry(const si_header &h, uint32_t t) {
  return si_geom{h.table[t].global_size, h.table[t].n_buckets, h.table[t].n_overflow, h.src_index, h.src_count, h.dst_index, h.dst_count};
}

// h = the image's header as the host has read and checked it (si_header_check): the kernels take the sizes from it, never
// from the image.  s.words[DINT_IMAGE_BAD_AT] = the violations found, s.words[2 t + 1] = table t's valid slots.
void dint_launch_image_check(const si_header &h, const uint8_t *d_buf, bool lock, dint_image_scratch s, hipStream_t st) {
  (void)hipMemsetAsync(s.words, 0, DINT_IMAGE_WORDS * sizeof(unsigned long long), st);
  uint32_t at = 0;
  for (uint32_t t = 0; t < h.n_tables; t++) {
    const uint32_t nb = si_blocks(h.table[t].n_buckets);
    if (nb) {
      hipLaunchKernelGGL(k_image_check, dim3(nb), dim3(SI_TB), 0, st, si_section(h, t, d_buf, lock), si_geometry(h, t), lock ? 1 : 0,
                         (uint32_t *)(s.words + DINT_IMAGE_BAD_AT), (sd_v2 *)s.blk + at);
      sd_launch_scan((const sd_v2 *)s.blk + at, nb, s.blk_off + at, s.words + 2 * t, st);
    }
    at += nb;
  }
}

void dint_launch_image_import(const dint_kv &kv, const si_header &h, const uint8_t *d_buf, const uint32_t *base, hipStream_t st) {
  const dint_mod H = dint_make_mod(h.dst_count);
  for (uint32_t t = 0; t < h.n_tables; t++) {
    const si_table &it = h.table[t];
    if (it.n_buckets + it.n_overflow == 0) continue;
    const uint32_t cb = si_copy_blocks(it.n_buckets + it.n_overflow, h.stride);
    if (h.stride == 256)
      hipLaunchKernelGGL(k_image_copy_in<256>, dim3(cb), dim3(SI_TB), 0, st, kv.h.tab[t], H, it.n_buckets, it.n_overflow, base[t], si_section(h, t, d_buf, false));
    else
      hipLaunchKernelGGL(k_image_copy_in<128>, dim3(cb), dim3(SI_TB), 0, st, kv.h.tab[t], H, it.n_buckets, it.n_overflow, base[t], si_section(h, t, d_buf, false));
  }
}

void dint_launch_image_lock_in(uint2 *tbl, uint64_t n_local, const si_header &h, const uint8_t *d_buf, hipStream_t st) {
  const uint64_t n = h.table[0].n_buckets;
  if (!n) return;
  hipLaunchKernelGGL(k_image_lock_in, dim3(si_blocks(n)), dim3(SI_TB), 0, st, tbl, n_local, dint_make_mod(h.dst_count), n, si_section(h, 0, d_buf, true));
}

// what a workload's image looks like: tables, stride, value size; false = a workload without tables
bool dint_image_shape(uint32_t workload, uint32_t *n_tables, uint32_t *stride, uint32_t *val_size) {
  switch (workload) {
    case DINT_WL_FASST:
    case DINT_WL_2PL: *n_tables = 1; *stride = SI_LOCK_STRIDE; *val_size = 0; return true;
    case DINT_WL_STORE: *n_tables = 1; *stride = 256; *val_size = 40; return true;
    case DINT_WL_TATP: *n_tables = 5; *stride = 256; *val_size = 40; return true;
    case DINT_WL_SMALLBANK: *n_tables = 2; *stride = 128; *val_size = 8; return true;
    default: return false;
  }
}

// ---- the host form (include/dint_driver.h): the same state_image.h rule over an image in host memory ------------------------
extern "C" int dint_state_image_check_host(const void *image, uint64_t bytes) {
  char msg[256];
  auto refuse = [&](const char *what, int table, long long at) {
    if (table < 0) snprintf(msg, sizeof msg, "image refused: %s", what);
    else snprintf(msg, sizeof msg, "image refused: %s (table %d, entry %lld)", what, table, at);
    dint_set_last_error(msg);
    return (int)DINT_EINVAL;
  };
  if (!image || bytes < SI_HEADER_BYTES) return refuse("shorter than its header", -1, 0);
  si_header h;
  memcpy(&h, image, sizeof h);
  uint32_t n_tables = 0, stride = 0, val_size = 0;
  if (h.magic != SI_MAGIC || h.version != SI_VERSION) return refuse("not a state image of this version", -1, 0);
  if (!dint_image_shape(h.workload, &n_tables, &stride, &val_size)) return refuse("a workload without tables", -1, 0);
  const bool lock = stride == SI_LOCK_STRIDE;
  if (h.n_tables != n_tables || h.stride != stride || h.val_size != val_size) return refuse("tables, stride or value size are not the workload's", -1, 0);
  if (uint32_t bad = si_header_check(h, bytes, lock)) return refuse(si_bad_name(bad), -1, 0);
  const uint8_t *p = (const uint8_t *)image;
  for (uint32_t t = 0; t < h.n_tables; t++) {
    const si_host_image im(h, t, p, lock);
    const si_geom g = si_geometry(h, t);
    for (uint64_t b = 0; b < h.table[t].n_buckets; b++) {
      uint64_t rows = 0;
      const uint32_t bad = lock ? si_check_slot(im, b, g) : si_check_bucket(im, b, g, &rows);
      if (bad) return refuse(si_bad_name(bad), (int)t, (long long)b);
    }
  }
  return 0;
}
