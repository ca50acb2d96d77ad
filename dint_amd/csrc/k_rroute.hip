// k_rroute.hip -- a list of canonical 64-byte records routed to the shards of another layout (dint_records_route, include/dint_abi.h;
// the rule: state_route.h): the STABLE partition of the list by home shard, in three stages like the other state calls.
//
//   k_rroute_count    one thread per record: key and table byte -> home (the table is range-checked first); the tile's records per
//                     home from wave ballots, summed over the tile's waves, to cnt[home][tile] (shard-major, so that ONE exclusive
//                     scan gives every (shard, tile) its first record).  A record without a home lowers words[0] to its index.
//   k_state_scan      state_dev.h's one-workgroup scan over the H x tiles counts; k_rroute_offsets gathers the H + 1 offsets
//   (host)            reads words[0] and the offsets in the call's one synchronisation; launches the write stage only for a good list
//   k_rroute_write    a tile of RR_TILE records: every lane loads its four 16-byte vectors (lane v: record v / 4, quarter v % 4 -- all
//                     loads before the first store), the tile is staged in LDS in input order, the homes are computed AGAIN from the
//                     staged keys (8 + 1 bytes of a record that is in LDS anyway and a dozen integer operations, against n bytes
//                     written and read back through HBM for a home[] array), the rank of a record among its home's records of the
//                     tile comes from wave ballots plus the per-wave counts of the waves below (k_route.hip k_route_pack's scheme), the
//                     tile is rewritten home-major in LDS from the registers, and leaves as 16-byte vectors: consecutive lanes write
//                     consecutive vectors of a home's run, so a run of the tile is one contiguous stream.  No atomic decides a
//                     position: two runs write the same bytes.
// 47 KB of LDS per workgroup of 512 (three per compute unit), 16 VGPRs of staged vectors, no scratch memory.  The permuting
// ds_write_b128 is 2-way conflicted at worst: the 8 lanes of a group hold two records, which share their 16 banks when their
// positions have the same parity.
// Nothing in a record can send an access outside the two buffers and the scratch: a home is < H <= 255 by construction, a record
// without one takes no part, positions are bounded by the tile and every store by n.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/dint_abi.h"
#include "../../include/dint_driver.h"
#include "dint_kv.h"
#include "state_dev.h"
#include "state_route.h"

#define RR_TB RR_TILE  // threads per workgroup: one per record of the tile, four vectors each in the write stage
#define RR_WAVES (RR_TB / 64u)
#define RR_BINS 256u   // LDS bins per wave: homes 0 .. 254
static_assert(RR_MAX_SHARDS < RR_BINS && RR_TILE * 64u + RR_WAVES * RR_BINS * 4u + RR_BINS * 16u + RR_TILE * 3u + 64u <= 65536u, "a workgroup stays within 64 KB of LDS");

__device__ static inline uint64_t rr_vec_key(const sd_v4 &v0) { return (uint64_t)v0.x | ((uint64_t)v0.y << 32); }

// the rank of this lane's record among the records of its home in its wave; wc[home] = the wave's records of that home (wc: the
// wave's RR_BINS words, zero before).  Every lane of the wave calls.
__device__ static inline uint32_t rr_wave_rank(bool valid, uint32_t h, uint32_t *wc) {
  const uint32_t lane = threadIdx.x & 63;
  uint32_t rank = 0;
  for (uint64_t todo = __ballot(valid); todo;) {
    const int l = __ffsll((unsigned long long)todo) - 1;
    const uint32_t hh = (uint32_t)__builtin_amdgcn_readlane(h, l);
    const uint64_t m = __ballot(valid && h == hh);
    if (valid && h == hh) rank = (uint32_t)__popcll(m & lanemask_lt());
    if ((int)lane == l) wc[hh] = (uint32_t)__popcll(m);
    todo &= ~m;
  }
  return rank;
}

// cnt[h * tiles + b] = tile b's records of home h; words[0] = min(words[0], index of a record without a home)
__global__ void __launch_bounds__(RR_TB)
k_rroute_count(const sd_v4 *__restrict__ rec, uint64_t n, rr_geom g, uint32_t tiles, uint32_t *__restrict__ cnt, unsigned long long *words) {
  __shared__ uint32_t Wc[RR_WAVES][RR_BINS];
  const uint32_t t = threadIdx.x, wave = t >> 6, b = blockIdx.x;
  for (uint32_t k = t; k < RR_WAVES * RR_BINS; k += RR_TB) (&Wc[0][0])[k] = 0;
  __syncthreads();
  const uint64_t i = (uint64_t)b * RR_TILE + t;
  bool valid = i < n;
  uint32_t h = 0;
  if (valid) {
    const sd_v4 v0 = rec[i * 4], v3 = rec[i * 4 + 3];
    h = rr_home(rr_vec_key(v0), rr_word_table(v3.y), g);
    if (h == RR_NO_HOME) {
      atomicMin(words, (unsigned long long)i);
      valid = false;
      h = 0;
    }
  }
  rr_wave_rank(valid, h, Wc[wave]);
  __syncthreads();
  if (t < g.n_shards) {
    uint32_t c = 0;
    for (uint32_t k = 0; k < RR_WAVES; k++) c += Wc[k][t];
    cnt[(size_t)t * tiles + b] = c;
  }
}

// words[2 + h] = offsets[h] (h < H), words[2 + H] = the scan's total
__global__ void __launch_bounds__(256) k_rroute_offsets(const uint64_t *__restrict__ off, uint32_t tiles, uint32_t H, unsigned long long *words) {
  const uint32_t t = threadIdx.x;
  if (t < H) words[2 + t] = off[(size_t)t * tiles];
  else if (t == H) words[2 + H] = words[1];
}

__global__ void __launch_bounds__(RR_TB)
k_rroute_write(const sd_v4 *__restrict__ rec, uint64_t n, rr_geom g, uint32_t tiles, const uint64_t *__restrict__ off, sd_v4 *__restrict__ out) {
  __shared__ sd_v4 S[RR_TILE * 4];            // the tile: input order, then home-major
  __shared__ uint32_t Wc[RR_WAVES][RR_BINS];  // records per wave and home
  __shared__ uint32_t Cnt[RR_BINS], Loff[RR_BINS];  // of the tile per home: records, first position
  __shared__ uint64_t Gb[RR_BINS];            // ... first record in the output
  __shared__ uint16_t Pos[RR_TILE];           // record -> position (0xFFFF: takes no part)
  __shared__ uint8_t Hs[RR_TILE];             // position -> home
  __shared__ uint32_t Wtot[4];
  const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6, b = blockIdx.x;
  const uint64_t first = (uint64_t)b * RR_TILE;
  if (first >= n) return;  // (workgroup-uniform)
  const uint32_t tile_n = (uint32_t)min((uint64_t)RR_TILE, n - first), nv = tile_n * 4;
  const sd_v4 *gsrc = rec + first * 4;
  sd_v4 r[4];
#pragma unroll
  for (uint32_t j = 0; j < 4; j++) {
    const uint32_t v = t + RR_TB * j;
    if (v < nv) r[j] = gsrc[v];
  }
  for (uint32_t k = t; k < RR_WAVES * RR_BINS; k += RR_TB) (&Wc[0][0])[k] = 0;
  if (t < RR_BINS) Gb[t] = t < g.n_shards ? off[(size_t)t * tiles + b] : 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; j++) {
    const uint32_t v = t + RR_TB * j;
    if (v < nv) S[v] = r[j];
  }
  __syncthreads();
  bool valid = t < tile_n;
  uint32_t h = 0;
  if (valid) {
    const sd_v4 v0 = S[4 * t], v3 = S[4 * t + 3];
    h = rr_home(rr_vec_key(v0), rr_word_table(v3.y), g);
    if (h == RR_NO_HOME) {  // (never in a list that passed the count stage)
      valid = false;
      h = 0;
    }
  }
  const uint32_t rank = rr_wave_rank(valid, h, Wc[wave]);
  __syncthreads();  // every staged key has been read; the waves' counts are in
  uint32_t c = 0, before = 0;
  if (t < RR_BINS) {  // (waves 0 .. 3, whole)
    for (uint32_t k = 0; k < RR_WAVES; k++) c += Wc[k][t];
    uint32_t tot;
    before = wave_excl_scan_u32(c, &tot);
    if (lane == 0) Wtot[wave] = tot;
  }
  __syncthreads();
  if (t < RR_BINS) {
    for (uint32_t w = 0; w < wave; w++) before += Wtot[w];
    Cnt[t] = c;
    Loff[t] = before;
  }
  __syncthreads();
  uint32_t pos = 0xFFFFu;
  if (valid) {
    pos = Loff[h] + rank;
    for (uint32_t k = 0; k < wave; k++) pos += Wc[k][h];
    Hs[pos] = (uint8_t)h;  // (pos < the tile's records with a home <= RR_TILE)
  }
  Pos[t] = (uint16_t)pos;
  __syncthreads();
#pragma unroll
  for (uint32_t j = 0; j < 4; j++) {
    const uint32_t v = t + RR_TB * j;
    if (v < nv) {
      const uint32_t p = Pos[v >> 2];
      if (p < RR_TILE) S[p * 4 + (v & 3u)] = r[j];
    }
  }
  __syncthreads();
  const uint32_t placed4 = (Loff[RR_BINS - 1] + Cnt[RR_BINS - 1]) * 4;  // vectors of the records that take part
  const uint64_t n4 = n * 4;
#pragma unroll
  for (uint32_t j = 0; j < 4; j++) {
    const uint32_t v = t + RR_TB * j;
    if (v < placed4) {
      const uint32_t p = v >> 2, hh = Hs[p];
      const uint64_t dst = (Gb[hh] + (p - Loff[hh])) * 4 + (v & 3u);
      if (dst < n4) out[dst] = S[v];
    }
  }
}

void dint_launch_rroute_count(const rr_geom &g, const void *d_rec, uint64_t n, dint_rroute_scratch s, hipStream_t st) {
  const uint32_t tiles = (uint32_t)rr_tiles(n);
  (void)hipMemsetAsync(s.words, 0xFF, sizeof(unsigned long long), st);  // words[0] = RR_NO_INDEX
  hipLaunchKernelGGL(k_rroute_count, dim3(tiles), dim3(RR_TB), 0, st, (const sd_v4 *)d_rec, n, g, tiles, s.cnt, s.words);
  sd_launch_scan((const uint32_t *)s.cnt, tiles * g.n_shards, s.off, s.words + 1, st);
  hipLaunchKernelGGL(k_rroute_offsets, dim3(1), dim3(256), 0, st, (const uint64_t *)s.off, tiles, g.n_shards, s.words);
}

void dint_launch_rroute_write(const rr_geom &g, const void *d_rec, uint64_t n, dint_rroute_scratch s, void *d_out, hipStream_t st) {
  const uint32_t tiles = (uint32_t)rr_tiles(n);
  hipLaunchKernelGGL(k_rroute_write, dim3(tiles), dim3(RR_TB), 0, st, (const sd_v4 *)d_rec, n, g, tiles, (const uint64_t *)s.off, (sd_v4 *)d_out);
}

// ---- the host form (include/dint_driver.h): the same rule over caller-provided memory -------------------------------------------
extern "C" uint32_t dint_records_route_tile(void) { return RR_TILE; }

extern "C" int64_t dint_records_route_host(uint32_t workload, uint64_t n_rows, uint32_t dst_count, const void *rec, uint64_t n, void *out,
                                           uint64_t *offsets) {
  if (workload != DINT_WL_STORE && workload != DINT_WL_TATP && workload != DINT_WL_SMALLBANK) {
    dint_set_last_error("workload has no kv table");
    return DINT_ESTATE;
  }
  if (dst_count == 0 || dst_count > RR_MAX_SHARDS || !offsets || (n && (!rec || !out))) {
    dint_set_last_error("dst_count: 1 .. 255; offsets, and for n records both buffers");
    return DINT_EINVAL;
  }
  const uint8_t *src = (const uint8_t *)rec;
  uint8_t *dst = (uint8_t *)out;
  if (n && src < dst + n * 64 && dst < src + n * 64) {
    dint_set_last_error("the input and the output overlap");
    return DINT_EINVAL;
  }
  uint64_t hs[DINT_KV_MAX_TABLES];
  uint32_t val_size;
  rr_geom g;
  g.n_tables = dint_kv_hash_sizes(workload, n_rows, hs, &val_size);
  g.n_shards = dst_count;
  for (uint32_t t = 0; t < RR_MAX_TABLES; t++) g.mod[t] = dint_make_mod(hs[t]);
  try {
    std::vector<uint8_t> home(n);
    std::vector<uint64_t> at(dst_count + 1, 0);
    for (uint64_t i = 0; i < n; i++) {  // check + count: nothing is written before the whole list has been read
      uint64_t key;
      uint32_t w13;
      memcpy(&key, src + i * 64, 8);
      memcpy(&w13, src + i * 64 + offsetof(LrRecord, is_del), 4);
      const uint32_t h = rr_home(key, rr_word_table(w13), g);
      if (h == RR_NO_HOME) {
        char msg[160];
        snprintf(msg, sizeof msg, "record %llu has no home: its table byte names a table the workload has not; nothing was written", (unsigned long long)i);
        dint_set_last_error(msg);
        return DINT_EINVAL;
      }
      home[i] = (uint8_t)h;
      at[h + 1]++;
    }
    for (uint32_t h = 0; h < dst_count; h++) at[h + 1] += at[h];
    memcpy(offsets, at.data(), (size_t)(dst_count + 1) * sizeof(uint64_t));
    for (uint64_t i = 0; i < n; i++) memcpy(dst + at[home[i]]++ * 64, src + i * 64, 64);
  } catch (const std::bad_alloc &) {
    dint_set_last_error("out of host memory");
    return DINT_ENOMEM;
  }
  return (int64_t)n;
}
