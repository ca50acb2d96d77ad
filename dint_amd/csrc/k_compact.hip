// k_compact.hip -- an engine's tables and overflow pool compacted in place (include/dint_abi.h dint_state_compact, driven by
// engine.hip; the rule lives in state_compact.h, which the host form at the end of this file shares).  Not on a request's path.
//
//   (k_verify.hip's census first: the gate)
//   k_compact_count    workgroup = 256 consecutive buckets, the workgroups striding over the table.  A lane walks its chain
//                      (state_dev.h sd_bucket under state_image.h si_chain_walk): the bucket's rows into rows[], and per
//                      workgroup of buckets {overflow entries afterwards, buckets to rewrite} and {inline entries linked, buckets
//                      with a row}.  Read-only and bounded whatever the table holds, so it does not wait for the gate.
//   k_state_scan       twice over those pairs: every workgroup's first overflow entry, and the four totals.
//   k_compact_move     the same shape.  A lane's first overflow entry from the scan; rows 4 .. go to the staging buffer at their
//                      final index, the places of rows 0 .. 3 are remembered; then the four rows are loaded and only then the
//                      inline entry is stored.
//   k_compact_commit   staging -> pool entries [0, new top) in 16-byte vectors, {validw, next} of the tail zeroed, pool_top, the
//                      192 head words.
// Move and commit read every table's summed census and the totals on the device and do nothing when a table fails the gate or
// its staging buffer is too small: no host round trip, and a refused call writes not a byte.  No atomic but the census's claim;
// no table content makes a kernel read or write outside the tables and the staging buffer or loop without bound.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/dint_abi.h"
#include "../../include/dint_driver.h"
#include "dint_kernels.h"
#include "dint_kv.h"
#include "state_compact.h"
#include "state_dev.h"
#include "state_image.h"
#include "state_rehash.h"
#include "state_verify.h"

#define CP_TB SD_TB
#define CP_GRID DINT_STATE_VERIFY_GRID

static_assert(sizeof(dint_table_compact) == 8 * CP_WORDS && offsetof(dint_table_compact, rows) == 8 * CP_ROWS &&
              offsetof(dint_table_compact, entries_after) == 8 * CP_ENTRIES_AFTER && offsetof(dint_table_compact, overflow_after) == 8 * CP_OVERFLOW_AFTER &&
              offsetof(dint_table_compact, pool_top_after) == 8 * CP_TOP_AFTER && offsetof(dint_table_compact, holes_after) == 8 * CP_HOLES_AFTER &&
              offsetof(dint_table_compact, buckets_rewritten) == 8 * CP_REWRITTEN && offsetof(dint_table_compact, unaccounted_dropped) == 8 * CP_DROPPED &&
              offsetof(dint_table_compact, staging_bytes) == 8 * CP_STAGING_BYTES && offsetof(dint_table_compact, reserved) == 8 * CP_STAGE_NS,
              "the words of state_compact.h are the fields of dint_table_compact");
static_assert(DINT_COMPACT_DRY_RUN == DINT_COMPACT_DRY_RUN_BIT && CP_SUMS == 4 && SV_LISTS <= CP_TB, "one flag; a workgroup covers the head words");

// what the moving kernels need to decide, on the device, whether the call goes ahead
struct cp_gate {
  const unsigned long long *census;  // [n_tables][SV_WORDS] the summed census of every table
  const unsigned long long *sums;    // [n_tables][CP_SUMS] the count stage's totals
  uint32_t n_tables;
  uint32_t stage_cap[DINT_KV_MAX_TABLES];  // entries each table's staging buffer holds
};
__device__ static inline bool cp_dev_go(const cp_gate &g) {
  bool ok = true;
  for (uint32_t t = 0; t < g.n_tables; t++)
    ok = ok && cp_gate_ok((const uint64_t *)g.census + (size_t)SV_WORDS * t) && g.sums[(size_t)CP_SUMS * t + CP_SUM_OVERFLOW] <= g.stage_cap[t];
  return ok;
}

__global__ void __launch_bounds__(CP_TB) k_compact_count(kv_tab t, uint32_t nb, uint32_t *__restrict__ rows, sd_v2 *__restrict__ blk_a,
                                                         sd_v2 *__restrict__ blk_b) {
  __shared__ uint32_t red[CP_TB / 64][CP_SUMS];
  const uint32_t tid = threadIdx.x;
  for (uint32_t blk = blockIdx.x; blk < nb; blk += gridDim.x) {  // (uniform in the workgroup)
    const uint64_t b = (uint64_t)blk * CP_TB + tid;
    uint32_t v[CP_SUMS] = {0, 0, 0, 0};
    if (b < t.n_local) {
      const cp_count c = cp_count_bucket(sd_bucket_at(t, b));
      const uint32_t k = c.ok ? c.k : 0u;  // (a chain that cannot be walked: the gate refuses the call)
      rows[b] = k;
      v[CP_SUM_OVERFLOW] = sr_overflow(k);
      v[CP_SUM_REWRITTEN] = c.rewritten;
      v[CP_SUM_INLINE_LINKED] = c.inline_linked;
      v[CP_SUM_NONEMPTY] = k != 0;
    }
    __syncthreads();  // (the previous round's readers of red are done)
    sd_block_sum(red, v);
    if (tid == 0) {
      blk_a[blk] = sd_v2{sd_block_total(red, CP_SUM_OVERFLOW), sd_block_total(red, CP_SUM_REWRITTEN)};
      blk_b[blk] = sd_v2{sd_block_total(red, CP_SUM_INLINE_LINKED), sd_block_total(red, CP_SUM_NONEMPTY)};
    }
  }
}

// the accessor of state_compact.h cp_move_bucket over a bucket in HBM; NW = 8-byte words of a value
template <uint32_t NW>
struct cp_dev_bucket {
  sd_bucket ch;
  uint8_t *stage;
  __device__ inline uint32_t head() const { return ch.head(); }
  __device__ inline bool link_ok(uint32_t link) const { return ch.link_ok(link); }
  __device__ inline void links(uint32_t link, uint32_t &validw, uint32_t &next) const { ch.links(link, validw, next); }
  __device__ inline void stage_row(uint32_t src_link, uint32_t src_slot, uint32_t pool, uint32_t slot) const {
    const uint8_t *s = kv_entry_ptr(ch.t, ch.b, src_link);
    uint8_t *d = stage + (size_t)pool * ch.t.stride;
    const uint64_t key = *(const KV_G(uint64_t) *)(s + 8u * src_slot);
    const uint32_t ver = *(const KV_G(uint32_t) *)(s + 32u + 4u * src_slot);
    uint64_t v[NW];
#pragma unroll
    for (uint32_t i = 0; i < NW; i++) v[i] = *(const KV_G(uint64_t) *)(s + KV_VAL_OFF + 8u * (NW * src_slot + i));
    *(KV_G(uint64_t) *)(d + 8u * slot) = key;
    *(KV_G(uint32_t) *)(d + 32u + 4u * slot) = ver;
#pragma unroll
    for (uint32_t i = 0; i < NW; i++) *(KV_G(uint64_t) *)(d + KV_VAL_OFF + 8u * (NW * slot + i)) = v[i];
  }
  __device__ inline void stage_links(uint32_t pool, uint32_t validw, uint32_t next) const {
    *(KV_G(sd_v2) *)(stage + (size_t)pool * ch.t.stride + KV_VALID_OFF) = sd_v2{validw, next};
  }
  __device__ inline void inline_write(const cp_loc (&loc)[4], uint32_t m, uint32_t validw, uint32_t next, uint32_t head) const {
    uint8_t *d = kv_entry_ptr(ch.t, ch.b, KV_INLINE);
    uint64_t key[4], v[4][NW];
    uint32_t ver[4];
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) {  // every load ...
      key[i] = 0;
      ver[i] = 0;
#pragma unroll
      for (uint32_t j = 0; j < NW; j++) v[i][j] = 0;
      if (i < m) {
        const uint8_t *s = kv_entry_ptr(ch.t, ch.b, loc[i].link);
        key[i] = *(const KV_G(uint64_t) *)(s + 8u * loc[i].slot);
        ver[i] = *(const KV_G(uint32_t) *)(s + 32u + 4u * loc[i].slot);
#pragma unroll
        for (uint32_t j = 0; j < NW; j++) v[i][j] = *(const KV_G(uint64_t) *)(s + KV_VAL_OFF + 8u * (NW * loc[i].slot + j));
      }
    }
    KV_G(sd_v4) *h = (KV_G(sd_v4) *)d;  // ... before the first store; lockw (the last word of the link vector) is not written
    h[0] = sd_v4{(uint32_t)key[0], (uint32_t)(key[0] >> 32), (uint32_t)key[1], (uint32_t)(key[1] >> 32)};
    h[1] = sd_v4{(uint32_t)key[2], (uint32_t)(key[2] >> 32), (uint32_t)key[3], (uint32_t)(key[3] >> 32)};
    h[2] = sd_v4{ver[0], ver[1], ver[2], ver[3]};
    *(KV_G(sd_v2) *)(d + KV_VALID_OFF) = sd_v2{validw, next};
    *(KV_G(uint32_t) *)(d + offsetof(kv_hdr, head)) = head;
#pragma unroll
    for (uint32_t i = 0; i < 4; i++)
#pragma unroll
      for (uint32_t j = 0; j < NW; j++) *(KV_G(uint64_t) *)(d + KV_VAL_OFF + 8u * (NW * i + j)) = v[i][j];
  }
};

template <uint32_t NW>
__global__ void __launch_bounds__(CP_TB) k_compact_move(kv_tab t, uint32_t table, uint32_t nb, const uint32_t *__restrict__ rows,
                                                        const uint64_t *__restrict__ blk_off, uint8_t *stage, cp_gate g) {
  __shared__ uint32_t red[CP_TB / 64];
  if (!cp_dev_go(g)) return;  // (the whole grid)
  const uint32_t tid = threadIdx.x;
  const uint64_t need = g.sums[(size_t)CP_SUMS * table + CP_SUM_OVERFLOW];  // (<= stage_cap[table]: cp_dev_go)
  for (uint32_t blk = blockIdx.x; blk < nb; blk += gridDim.x) {
    const uint64_t b = (uint64_t)blk * CP_TB + tid;
    const uint32_t k = b < t.n_local ? rows[b] : 0u, ovf = sr_overflow(k);
    __syncthreads();  // (the previous round's readers of red are done)
    const uint64_t base = blk_off[blk] + sd_block_excl_scan(red, ovf);
    if (b >= t.n_local || base + ovf > need) continue;  // (never the second: the scan summed the same counts)
    const cp_dev_bucket<NW> a = {sd_bucket_at(t, b), stage};
    cp_move_bucket(a, k, (uint32_t)base);
  }
}

__global__ void __launch_bounds__(CP_TB) k_compact_commit(kv_tab t, uint32_t table, const uint8_t *__restrict__ stage, cp_gate g) {
  if (!cp_dev_go(g)) return;
  const uint64_t new_top = g.sums[(size_t)CP_SUMS * table + CP_SUM_OVERFLOW];
  if (new_top > t.pool_cap) return;  // (never: every overflow entry afterwards was one before)
  const uint32_t old_top = sv_top((uint32_t)g.census[(size_t)SV_WORDS * table + SV_POOL_TOP], t.pool_cap);  // (the census's copy: pool_top is stored below)
  const uint64_t gid = (uint64_t)blockIdx.x * CP_TB + threadIdx.x, step = (uint64_t)gridDim.x * CP_TB;
  uint8_t *pool = t.entries + t.n_local * (uint64_t)t.stride;
  const uint64_t n_vec = new_top * (t.stride / 16u);
  for (uint64_t i = gid; i < n_vec; i += step) ((KV_G(sd_v4) *)pool)[i] = ((const KV_G(sd_v4) *)stage)[i];
  for (uint64_t p = new_top + gid; p < old_top; p += step) *(KV_G(sd_v2) *)(pool + p * t.stride + KV_VALID_OFF) = sd_v2{0u, 0u};
  if (blockIdx.x == 0) {
    const uint32_t tid = threadIdx.x;
    if (tid < SV_LISTS) {
      unsigned long long *hw = tid < KV_NLISTS ? t.free_head + tid : t.pend_head + (tid - KV_NLISTS);
      const unsigned long long old = *(const volatile KV_G(unsigned long long) *)hw;
      *hw = ((old >> 32) + 1ull) << 32;
    }
    if (tid == 0) *t.pool_top = (uint32_t)new_top;
  }
}

// ------------------------------------------------------------------------------------------------------ host side
static uint32_t cp_nb(const kv_tab &t) { return (uint32_t)((t.n_local + CP_TB - 1) / CP_TB); }
static uint32_t cp_grid(uint64_t n) {
  const uint64_t nb = (n + CP_TB - 1) / CP_TB;
  return (uint32_t)(nb < 1 ? 1 : nb > CP_GRID ? CP_GRID : nb);
}
void dint_compact_free(dint_compact_scratch &s) {
  hipFree(s.rows); hipFree(s.blk_a); hipFree(s.blk_b); hipFree(s.blk_off); hipFree(s.blk_junk); hipFree(s.sums);
  for (uint8_t *p : s.stage) hipFree(p);
  s = dint_compact_scratch{};
}
int dint_compact_alloc(const dint_kv &kv, dint_compact_scratch &s) {
  if (s.sums) return 0;
  uint64_t n_rows = 0, nb = 0;
  for (uint32_t t = 0; t < kv.n_tables; t++) {
    n_rows += kv.h.tab[t].n_local;
    nb += cp_nb(kv.h.tab[t]);
  }
  const bool ok = hipMalloc((void **)&s.rows, n_rows * sizeof(uint32_t)) == hipSuccess && hipMalloc((void **)&s.blk_a, nb * sizeof(sd_v2)) == hipSuccess &&
                  hipMalloc((void **)&s.blk_b, nb * sizeof(sd_v2)) == hipSuccess && hipMalloc((void **)&s.blk_off, nb * sizeof(uint64_t)) == hipSuccess &&
                  hipMalloc((void **)&s.blk_junk, nb * sizeof(uint64_t)) == hipSuccess &&
                  hipMalloc((void **)&s.sums, (size_t)DINT_KV_MAX_TABLES * CP_SUMS * sizeof(unsigned long long)) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    dint_compact_free(s);
    dint_set_last_error("table compact: out of device memory for the row counts");
    return DINT_ENOMEM;
  }
  return 0;
}

// the census, the count stage and the scans; unless dry, move and commit behind them.  ev (may be null): five events
static void cp_launch(const dint_kv &kv, dint_verify_scratch vs, const dint_compact_scratch &s, bool dry, hipStream_t st, hipEvent_t *ev) {
  if (ev) (void)hipEventRecord(ev[0], st);
  dint_launch_state_verify(kv, vs, 0, st);
  if (ev) (void)hipEventRecord(ev[1], st);
  cp_gate g;
  memset(&g, 0, sizeof g);
  g.census = vs.out;
  g.sums = s.sums;
  g.n_tables = kv.n_tables;
  uint64_t row_at = 0, blk_at = 0;
  for (uint32_t t = 0; t < kv.n_tables; t++) {
    const kv_tab &tb = kv.h.tab[t];
    const uint32_t nb = cp_nb(tb);
    g.stage_cap[t] = s.stage_cap[t];
    hipLaunchKernelGGL(k_compact_count, dim3(nb < CP_GRID ? nb : CP_GRID), dim3(CP_TB), 0, st, tb, nb, s.rows + row_at, (sd_v2 *)s.blk_a + blk_at,
                       (sd_v2 *)s.blk_b + blk_at);
    sd_launch_scan<sd_v2>((const sd_v2 *)s.blk_a + blk_at, nb, s.blk_off + blk_at, s.sums + (size_t)CP_SUMS * t, st);
    sd_launch_scan<sd_v2>((const sd_v2 *)s.blk_b + blk_at, nb, s.blk_junk + blk_at, s.sums + (size_t)CP_SUMS * t + 2, st);
    row_at += tb.n_local;
    blk_at += nb;
  }
  if (ev) (void)hipEventRecord(ev[2], st);
  if (!dry) {
    row_at = blk_at = 0;
    for (uint32_t t = 0; t < kv.n_tables; t++) {
      const kv_tab &tb = kv.h.tab[t];
      const uint32_t nb = cp_nb(tb), grid = nb < CP_GRID ? nb : CP_GRID;
      if (s.stage_cap[t]) (void)hipMemsetAsync(s.stage[t], 0, (size_t)s.stage_cap[t] * tb.stride, st);  // (the call's stream, not the null stream)
      if (tb.val_size == 40)
        hipLaunchKernelGGL(k_compact_move<5>, dim3(grid), dim3(CP_TB), 0, st, tb, t, nb, (const uint32_t *)(s.rows + row_at),
                           (const uint64_t *)(s.blk_off + blk_at), s.stage[t], g);
      else
        hipLaunchKernelGGL(k_compact_move<1>, dim3(grid), dim3(CP_TB), 0, st, tb, t, nb, (const uint32_t *)(s.rows + row_at),
                           (const uint64_t *)(s.blk_off + blk_at), s.stage[t], g);
      row_at += tb.n_local;
      blk_at += nb;
    }
  }
  if (ev) (void)hipEventRecord(ev[3], st);
  if (!dry)
    for (uint32_t t = 0; t < kv.n_tables; t++) {
      const kv_tab &tb = kv.h.tab[t];
      const uint64_t vecs = (uint64_t)s.stage_cap[t] * (tb.stride / 16u);
      hipLaunchKernelGGL(k_compact_commit, dim3(cp_grid(vecs > tb.pool_cap ? vecs : tb.pool_cap)), dim3(CP_TB), 0, st, tb, t,
                         (const uint8_t *)s.stage[t], g);
    }
  if (ev) (void)hipEventRecord(ev[4], st);
}

static int cp_fail(int rc, const char *what) {
  dint_set_last_error(what);
  return rc;
}
// the words of every table as the caller sees them.  h[t] = the census words as summed (not yet finished), sums[t] = the count
// stage's totals.  Returns 0 or DINT_ESTATE (a table fails the gate: every table reports its census and zeros)
static int cp_finish(uint64_t (*h)[CP_WORDS], const uint64_t (*sums)[CP_SUMS], const dint_kv &kv, dint_table_compact *out) {
  int rc = 0;
  bool all_ok = true;
  for (uint32_t t = 0; t < kv.n_tables; t++) all_ok = all_ok && cp_gate_ok(h[t]);
  for (uint32_t t = 0; t < kv.n_tables; t++) {
    if (!cp_gate_ok(h[t]) && !rc) {
      char msg[256];
      snprintf(msg, sizeof msg, "table %u: %llu bad chains, %llu cross-linked entries, %llu entries linked beyond the pool's top, %llu bad list links, "
               "%llu stray valid entries, %llu misplaced rows, %llu odd valid bytes: nothing compacted", t, (unsigned long long)h[t][SV_BAD_CHAINS],
               (unsigned long long)h[t][SV_CROSS], (unsigned long long)h[t][SV_BEYOND_TOP], (unsigned long long)h[t][SV_LIST_BAD_LINKS],
               (unsigned long long)h[t][SV_STRAY_ENTRIES], (unsigned long long)h[t][SV_MISPLACED], (unsigned long long)h[t][SV_ODD_BYTES]);
      dint_set_last_error(msg);
      rc = DINT_ESTATE;
    }
    sv_report_finish(h[t], false);
    cp_report_finish(h[t], sums[t], kv.h.tab[t].stride, all_ok);
  }
  memcpy(out, h, (size_t)kv.n_tables * sizeof(dint_table_compact));
  return rc;
}

int dint_compact_run(const dint_kv &kv, dint_verify_scratch vs, dint_compact_scratch &s, uint32_t flags, hipStream_t st, dint_table_compact *out,
                     hipEvent_t *ev) {
  const bool dry = (flags & DINT_COMPACT_DRY_RUN) != 0;
  for (int attempt = 0; attempt < 2; attempt++) {
    cp_launch(kv, vs, s, dry, st, ev);
    hipError_t err = hipGetLastError();
    uint64_t census[DINT_KV_MAX_TABLES][SV_WORDS], sums[DINT_KV_MAX_TABLES][CP_SUMS], h[DINT_KV_MAX_TABLES][CP_WORDS];
    if (err == hipSuccess) err = hipMemcpyAsync(census, vs.out, sizeof census, hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipMemcpyAsync(sums, s.sums, sizeof sums, hipMemcpyDeviceToHost, st);
    const hipError_t serr = hipStreamSynchronize(st);  // (the one synchronisation of the call, unless the staging buffer has to grow)
    if (err == hipSuccess) err = serr;
    if (err != hipSuccess) {
      char msg[160];
      snprintf(msg, sizeof msg, "table compact: %s", hipGetErrorString(err));
      return cp_fail(DINT_EHIP, msg);
    }
    memset(h, 0, sizeof h);
    for (uint32_t t = 0; t < kv.n_tables; t++) memcpy(h[t], census[t], sizeof census[t]);
    if (int rc = cp_finish(h, sums, kv, out)) return rc;
    bool fits = true;
    for (uint32_t t = 0; t < kv.n_tables; t++) fits = fits && sums[t][CP_SUM_OVERFLOW] <= s.stage_cap[t];
    if (dry || fits) return 0;  // (fits: the kernels saw the same numbers and went ahead)
    // the kernels did nothing: a staging buffer of exactly what each table needs, and the whole call again
    for (uint32_t t = 0; t < kv.n_tables; t++) {
      const uint64_t need = sums[t][CP_SUM_OVERFLOW];
      if (need <= s.stage_cap[t]) continue;
      hipFree(s.stage[t]);
      s.stage[t] = nullptr;
      s.stage_cap[t] = 0;
      if (need > 0xFFFFFFF0ull || hipMalloc((void **)&s.stage[t], need * kv.h.tab[t].stride) != hipSuccess) {
        (void)hipGetLastError();
        s.stage[t] = nullptr;
        return cp_fail(DINT_ENOMEM, "table compact: out of device memory for the staging buffer; nothing was written");
      }
      s.stage_cap[t] = (uint32_t)need;
    }
  }
  return cp_fail(DINT_ESTATE, "table compact: the tables changed during the call");
}

// ---- the forms over caller-provided memory (include/dint_driver.h) -----------------------------------------------------------
extern "C" int dint_state_compact_view(int32_t device, const dint_tables_view *view, dint_table_compact *out, uint32_t cap_tables, uint32_t flags,
                                       void *stream) {
  if (flags & ~DINT_COMPACT_DRY_RUN) return cp_fail(DINT_EINVAL, "unknown flags");
  dint_kv kv;
  if (int rc = dint_view_kv(view, out, cap_tables, &kv)) return rc;
  if (hipSetDevice(device) != hipSuccess) return cp_fail(DINT_EHIP, "table view: no such device");
  dint_verify_scratch vs{};
  dint_compact_scratch cs{};
  int rc = dint_verify_alloc(kv, vs, 0);
  if (!rc) rc = dint_compact_alloc(kv, cs);
  if (!rc) rc = dint_compact_run(kv, vs, cs, flags, (hipStream_t)stream, out, nullptr);
  dint_verify_free(vs);
  dint_compact_free(cs);
  return rc ? rc : (int)kv.n_tables;
}

// the accessor of state_compact.h over host memory (the words at any alignment the view's check let through)
struct cp_host_bucket {
  const kv_tab &t;
  uint64_t b;
  uint8_t *stage;
  uint8_t *e(uint32_t link) const { return kv_entry_ptr(t, b, link); }
  uint32_t head() const { return si_ld32(e(KV_INLINE) + offsetof(kv_hdr, head)); }
  bool link_ok(uint32_t link) const { return link - 2u < t.pool_cap; }
  void links(uint32_t link, uint32_t &validw, uint32_t &next) const {
    validw = si_ld32(e(link) + KV_VALID_OFF);
    next = si_ld32(e(link) + offsetof(kv_hdr, next));
  }
  static void row(uint8_t *d, uint32_t slot, const uint8_t *s, uint32_t src_slot, uint32_t val_size) {
    memcpy(d + 8u * slot, s + 8u * src_slot, 8);
    memcpy(d + 32u + 4u * slot, s + 32u + 4u * src_slot, 4);
    memcpy(d + KV_VAL_OFF + val_size * slot, s + KV_VAL_OFF + val_size * src_slot, val_size);
  }
  void stage_row(uint32_t src_link, uint32_t src_slot, uint32_t pool, uint32_t slot) const {
    row(stage + (size_t)pool * t.stride, slot, e(src_link), src_slot, t.val_size);
  }
  void stage_links(uint32_t pool, uint32_t validw, uint32_t next) const {
    uint8_t *d = stage + (size_t)pool * t.stride;
    memcpy(d + KV_VALID_OFF, &validw, 4);
    memcpy(d + offsetof(kv_hdr, next), &next, 4);
  }
  void inline_write(const cp_loc (&loc)[4], uint32_t m, uint32_t validw, uint32_t next, uint32_t head) const {
    uint8_t tmp[KV_VAL_OFF + 4 * 40];  // keys, versions and values of the four slots: every load before the first store
    memset(tmp, 0, sizeof tmp);
    for (uint32_t i = 0; i < m; i++) row(tmp, i, e(loc[i].link), loc[i].slot, t.val_size);
    uint8_t *d = e(KV_INLINE);
    memcpy(d, tmp, KV_VALID_OFF);
    memcpy(d + KV_VALID_OFF, &validw, 4);
    memcpy(d + offsetof(kv_hdr, next), &next, 4);
    memcpy(d + offsetof(kv_hdr, head), &head, 4);
    memcpy(d + KV_VAL_OFF, tmp + KV_VAL_OFF, 4u * t.val_size);
  }
};

extern "C" int dint_state_compact_view_host(const dint_tables_view *view, dint_table_compact *out, uint32_t cap_tables, uint32_t flags) {
  if (flags & ~DINT_COMPACT_DRY_RUN) return cp_fail(DINT_EINVAL, "unknown flags");
  dint_kv kv;
  if (int rc = dint_view_kv(view, out, cap_tables, &kv)) return rc;
  dint_table_verify census[DINT_KV_MAX_TABLES];
  if (int rc = dint_state_verify_view_host(view, census, DINT_KV_MAX_TABLES, 0); rc < 0) return rc;
  uint64_t h[DINT_KV_MAX_TABLES][CP_WORDS], sums[DINT_KV_MAX_TABLES][CP_SUMS];
  memset(h, 0, sizeof h);
  memset(sums, 0, sizeof sums);
  std::vector<uint32_t> rows[DINT_KV_MAX_TABLES];
  std::vector<uint8_t> stage[DINT_KV_MAX_TABLES];
  try {
    for (uint32_t ti = 0; ti < kv.n_tables; ti++) {
      const kv_tab &t = kv.h.tab[ti];
      memcpy(h[ti], &census[ti], sizeof census[ti]);
      rows[ti].assign((size_t)t.n_local, 0u);
      for (uint64_t b = 0; b < t.n_local; b++) {
        const cp_host_bucket a = {t, b, nullptr};
        const cp_count c = cp_count_bucket(a);
        const uint32_t k = c.ok ? c.k : 0u;
        rows[ti][b] = k;
        sums[ti][CP_SUM_OVERFLOW] += sr_overflow(k);
        sums[ti][CP_SUM_REWRITTEN] += c.rewritten;
        sums[ti][CP_SUM_INLINE_LINKED] += c.inline_linked;
        sums[ti][CP_SUM_NONEMPTY] += k != 0;
      }
    }
    if (int rc = cp_finish(h, sums, kv, out)) return rc;
    if (flags & DINT_COMPACT_DRY_RUN) return (int)kv.n_tables;
    for (uint32_t ti = 0; ti < kv.n_tables; ti++)  // (every buffer before the first write)
      stage[ti].assign((size_t)sums[ti][CP_SUM_OVERFLOW] * kv.h.tab[ti].stride, (uint8_t)0);
  } catch (const std::bad_alloc &) {
    return cp_fail(DINT_ENOMEM, "table compact: out of memory for the staging buffer; nothing was written");
  }
  for (uint32_t ti = 0; ti < kv.n_tables; ti++) {
    const kv_tab &t = kv.h.tab[ti];
    const uint32_t new_top = (uint32_t)sums[ti][CP_SUM_OVERFLOW], old_top = sv_top((uint32_t)h[ti][SV_POOL_TOP], t.pool_cap);
    uint32_t base = 0;
    for (uint64_t b = 0; b < t.n_local; b++) {
      const cp_host_bucket a = {t, b, stage[ti].data()};
      cp_move_bucket(a, rows[ti][b], base);
      base += sr_overflow(rows[ti][b]);
    }
    uint8_t *pool = t.entries + t.n_local * (uint64_t)t.stride;
    if (new_top) memcpy(pool, stage[ti].data(), (size_t)new_top * t.stride);
    for (uint32_t p = new_top; p < old_top; p++) memset(pool + (size_t)p * t.stride + KV_VALID_OFF, 0, 8);  // {validw, next}
    for (uint32_t l = 0; l < SV_LISTS; l++) {
      unsigned long long *hw = l < KV_NLISTS ? t.free_head + l : t.pend_head + (l - KV_NLISTS);
      *hw = ((*hw >> 32) + 1ull) << 32;
    }
    *t.pool_top = new_top;
  }
  return (int)kv.n_tables;
}
