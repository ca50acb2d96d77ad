// state_load_main.cc -- the bulk load's rule (dint_amd/csrc/state_load.h: what k_load.hip's kernels and the host forms of
// include/dint_driver.h run) as a stand-alone program for a sanitizer run.  Every table, row array and plan lives in a heap block of
// exactly its size.  It checks
//   placement   sl_plan_host + sl_build_host into a table that holds nothing against kv_insert<kv_host_mem> of the same rows in
//               order (dint_kv_core.h, the code the request path runs): per bucket the chain-order dump, the header walk (inline or
//               pool entry, valid words, chain length), pool_top; buckets of 0, 1, 4, 5, 8, 9 and 41 rows; a key held twice across
//               an entry boundary; 3 shards; 8-byte values
//   the jump    sl_lcg_jump against stepping
//   generation  sl_gen_sub tile by tile -- the tile's first state from the jump or from sl_tile_walk, the subscribers' states from
//               the draw rule alone, as k_load_gen does -- against dint_pop::generate (dint_populate.h), rows and order exact, for
//               every table of store, tatp and smallbank; the tile table against a plain serial run of the reference's draws
// Build and run (host code only; nothing of it is loaded into python):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/native/state_load_main.cc -o state_load_main
//   ./state_load_main
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "../../dint_amd/csrc/dint_populate.h"
#include "../../dint_amd/csrc/state_load.h"

// fasthash64(&key, 8, 0xdeadbeef) (lock_fasst/udp/utils.h:16-53), restated
static uint64_t mix(uint64_t h) {
  h ^= h >> 23;
  h *= 0x2127599bf4325c37ULL;
  h ^= h >> 47;
  return h;
}
static uint64_t hash_key(uint64_t key) {
  const uint64_t m = 0x880355f21e6d1965ULL;
  uint64_t h = 0xdeadbeefULL ^ (8 * m);
  h ^= mix(key);
  h *= m;
  return mix(h);
}

static int bad = 0;
#define CHECK(cond)                                 \
  do {                                              \
    if (!(cond)) {                                  \
      printf("line %d: %s\n", __LINE__, #cond);     \
      bad++;                                        \
    }                                               \
  } while (0)

struct table {  // a table that holds nothing, every array exactly its size
  kv_tab t{};
  uint32_t top = 0;
  unsigned long long lists[2 * KV_NLISTS];
  table(uint64_t n_local, uint32_t pool_cap, uint32_t val_size) {
    memset(lists, 0, sizeof lists);
    t.n_local = n_local;
    t.pool_cap = pool_cap;
    t.stride = val_size == 40 ? 256 : 128;
    t.val_size = val_size;
    t.entries = (uint8_t *)calloc((n_local + pool_cap) * t.stride, 1);
    t.pool_next = (uint32_t *)calloc(pool_cap ? pool_cap : 1, 4);
    t.pool_top = &top;
    t.free_head = lists;
    t.pend_head = lists + KV_NLISTS;
  }
  ~table() {
    free(t.entries);
    free(t.pool_next);
  }
  table(const table &) = delete;
};

// what a walk of bucket b sees: per entry {inline?, validw}, then the rows in chain order
struct walk {
  std::vector<uint32_t> shape;
  std::vector<uint64_t> keys;
  std::vector<uint32_t> vers;
  std::vector<uint8_t> vals;
  bool operator==(const walk &o) const { return shape == o.shape && keys == o.keys && vers == o.vers && vals == o.vals; }
};
static walk walk_bucket(const kv_tab &t, uint64_t b) {
  walk w;
  uint32_t cur = kv_entry_hdr(t, b, KV_INLINE)->head;
  for (uint32_t steps = 0; cur != KV_NULL && steps < KV_MAX_CHAIN + 1; steps++) {
    const uint8_t *e = kv_entry_ptr(t, b, cur);
    const kv_hdr *h = (const kv_hdr *)e;
    w.shape.push_back(cur == KV_INLINE);
    w.shape.push_back(h->validw);
    for (uint32_t i = 0; i < 4; i++)
      if (kv_valid(*h, i)) {
        w.keys.push_back(h->key[i]);
        w.vers.push_back(h->ver[i]);
        w.vals.insert(w.vals.end(), e + KV_VAL_OFF + i * t.val_size, e + KV_VAL_OFF + (i + 1) * t.val_size);
      }
    cur = h->next;
  }
  return w;
}

// rows whose home rows per LOCAL bucket of shard `index` are per[], shuffled over the buckets, with foreign rows among them when
// sharded; dup: the row that lands at r = 4 of bucket `dup_bucket` repeats the key at r = 3
static void placement_case(uint64_t hash_size, uint32_t index, uint32_t count, const std::vector<uint32_t> &per, uint32_t val_size, int dup_bucket) {
  const uint64_t n_local = (hash_size + count - 1) / count;
  CHECK(per.size() == n_local);
  std::vector<std::vector<uint64_t>> by(n_local);
  std::vector<uint64_t> foreign;
  for (uint64_t k = 1; ; k++) {  // keys by home bucket
    const uint64_t g = hash_key(k * 0x9E3779B97F4A7C15ull) % hash_size;
    bool full = true;
    for (uint64_t b = 0; b < n_local; b++) full = full && by[b].size() >= per[b];
    if (full && foreign.size() >= (count > 1 ? 9u : 0u)) break;
    if (g % count != index) {
      if (foreign.size() < 9) foreign.push_back(k * 0x9E3779B97F4A7C15ull);
      continue;
    }
    if (by[g / count].size() < per[g / count]) by[g / count].push_back(k * 0x9E3779B97F4A7C15ull);
  }
  if (dup_bucket >= 0) by[dup_bucket][4] = by[dup_bucket][3];
  // insertion order: round-robin over the buckets, so every bucket's rows are spread over the whole list; foreign rows in between
  std::vector<uint64_t> keys;
  for (uint32_t r = 0, more = 1; more; r++) {
    more = 0;
    for (uint64_t b = 0; b < n_local; b++)
      if (r < by[b].size()) {
        keys.push_back(by[b][r]);
        more = 1;
      }
    if (r < foreign.size()) keys.push_back(foreign[r]);
  }
  const uint64_t n = keys.size();
  uint64_t *hk = (uint64_t *)malloc(n * 8);
  uint32_t *hv = (uint32_t *)malloc(n * 4);
  uint8_t *hval = (uint8_t *)malloc(n * val_size);
  for (uint64_t i = 0; i < n; i++) {
    hk[i] = keys[i];
    hv[i] = (uint32_t)(1000 + i);
    for (uint32_t j = 0; j < val_size; j++) hval[i * val_size + j] = (uint8_t)(i * 7 + j);
  }
  uint32_t need = 0;
  for (uint32_t p : per) need += sr_overflow(p);
  table a(n_local, need, val_size), b(n_local, need, val_size);
  // lock words and counters share the entries with the rows: the load must leave them as they are
  for (uint64_t x = 0; x < n_local; x++) {
    kv_entry_hdr(a.t, x, KV_INLINE)->lockw = 0xA5000000u | (uint32_t)x;
    kv_entry_hdr(b.t, x, KV_INLINE)->lockw = 0xA5000000u | (uint32_t)x;
    if (val_size == 8) memset(a.t.entries + x * 128 + KV_SB_LOCK_OFF, 0x33, 32), memset(b.t.entries + x * 128 + KV_SB_LOCK_OFF, 0x33, 32);
  }
  std::vector<uint32_t> order;
  std::vector<uint64_t> bucket;
  const sl_place_result res = sl_plan_host(hk, n, hash_size, index, count, hash_key, order, bucket);
  CHECK(res.overflow_entries == need && !res.too_long);
  CHECK(res.foreign_rows == (count > 1 ? foreign.size() : 0) && res.rows_loaded + res.foreign_rows == n);
  sl_build_host(a.t, hk, hv, hval, n, order, bucket);
  for (uint64_t i = 0; i < n; i++) {  // the serial load
    const uint64_t g = hash_key(hk[i]) % hash_size;
    if (g % count != index) continue;
    CHECK(kv_insert<kv_host_mem>(b.t, g / count, hk[i], hval + i * val_size, hv[i]));
  }
  CHECK(a.top == b.top && a.top == need);
  uint32_t longest = 0;
  for (uint64_t x = 0; x < n_local; x++) {
    const walk wa = walk_bucket(a.t, x), wb = walk_bucket(b.t, x);
    CHECK(wa == wb);
    CHECK(wa.keys.size() == per[x]);
    longest = std::max<uint32_t>(longest, (uint32_t)wa.shape.size() / 2);
    CHECK(kv_entry_hdr(a.t, x, KV_INLINE)->lockw == (0xA5000000u | (uint32_t)x));
    if (val_size == 8)
      for (uint32_t j = 0; j < 32; j++) CHECK(a.t.entries[x * 128 + KV_SB_LOCK_OFF + j] == 0x33);
  }
  CHECK(res.longest_chain_entries == longest);
  if (dup_bucket >= 0) {  // the visible row of the doubled key is the one the serial load shows
    uint8_t va[40], vb[40];
    uint32_t ra = 0, rb = 0;
    CHECK(kv_get(a.t, dup_bucket, by[dup_bucket][3], va, &ra) && kv_get(b.t, dup_bucket, by[dup_bucket][3], vb, &rb));
    CHECK(ra == rb && !memcmp(va, vb, val_size));
  }
  // the pool's free and pend lists stay empty
  for (uint32_t l = 0; l < 2 * KV_NLISTS; l++) CHECK((uint32_t)a.lists[l] == KV_NULL);
  free(hk);
  free(hv);
  free(hval);
}

static void jump_cases() {
  const uint64_t ks[] = {0, 1, 2, 12, 17, (1ull << 20) + 3};
  for (uint64_t seed : {SL_SEED, 0ull, 0xFFFFFFFFFFFFFFFFull}) {
    uint64_t s = seed, at = 0;
    for (uint64_t k : ks) {
      for (; at < k; at++) sl_lcg_next(s);
      CHECK(sl_lcg_jump(seed, k) == s);
    }
  }
}

// the rows of `table` for n subscribers, tile by tile as the kernel goes
static void gen_tiled(uint32_t workload, uint32_t table, uint64_t n, std::vector<uint64_t> &keys, std::vector<uint8_t> &vals, uint32_t vs) {
  uint32_t which;
  const uint32_t group = sl_group(workload, table, &which), draws = sl_draws(group);
  sl_tiles tl;
  if (draws == SL_DRAWS_VAR) sl_tile_walk(group, tl, n);
  for (uint64_t s0 = 0; s0 < n; s0 += SL_TILE) {
    uint64_t st[SL_TILE];
    if (draws == SL_DRAWS_VAR) {
      uint64_t g = tl.state[s0 / SL_TILE];
      for (uint32_t i = 0; i < SL_TILE && s0 + i < n; i++) {
        st[i] = g;
        uint32_t r[2];
        sl_skip_sub(group, s0 + i, g, r);
      }
    } else {
      for (uint32_t i = 0; i < SL_TILE && s0 + i < n; i++) st[i] = sl_lcg_jump(SL_SEED, (uint64_t)draws * (s0 + i));
    }
    for (uint32_t i = 0; i < SL_TILE && s0 + i < n; i++) {
      uint64_t g = st[i];
      sl_gen_sub(group, s0 + i, g, [&](uint32_t w_, uint64_t key, const uint64_t *w) {
        if (w_ != which) return;
        keys.push_back(key);
        vals.insert(vals.end(), (const uint8_t *)w, (const uint8_t *)w + vs);
      });
    }
  }
}

static void generation_cases() {
  const uint64_t ns[] = {1, SL_TILE - 1, SL_TILE, SL_TILE + 1, 3 * SL_TILE + 7};
  const uint32_t wls[] = {DINT_WL_STORE, DINT_WL_TATP, DINT_WL_SMALLBANK}, nts[] = {1, 5, 2};
  for (int k = 0; k < 3; k++)
    for (uint64_t n : ns) {
      const uint32_t vs = wls[k] == DINT_WL_SMALLBANK ? 8 : 40;
      std::map<uint32_t, std::vector<uint64_t>> rk;
      std::map<uint32_t, std::vector<uint8_t>> rv;
      CHECK(dint_pop::generate(wls[k], n, [&](uint32_t table, const uint64_t *keys, const uint8_t *vals, uint64_t m) {
        rk[table].insert(rk[table].end(), keys, keys + m);
        rv[table].insert(rv[table].end(), vals, vals + m * vs);
        return 0;
      }) == 0);
      for (uint32_t t = 0; t < nts[k]; t++) {
        std::vector<uint64_t> keys;
        std::vector<uint8_t> vals;
        gen_tiled(wls[k], t, n, keys, vals, vs);
        CHECK(keys == rk[t]);
        CHECK(vals == rv[t]);
        CHECK(!keys.empty());
      }
    }
  // the tile tables against a plain serial run of the reference's draws (dint_populate.h pick_types and the loops of generate)
  const uint64_t n = 5 * SL_TILE + 3;
  sl_tiles ai, sf;
  sl_tile_walk(SL_G_AI, ai, 2 * SL_TILE);  // (continued below: a prefix stays a prefix)
  sl_tile_walk(SL_G_AI, ai, n);
  sl_tile_walk(SL_G_SFCF, sf, n);
  CHECK(ai.state.size() == n / SL_TILE + 1 && sf.state.size() == n / SL_TILE + 1);
  dint_pop::Lcg ga(0xdeadbeef), gs(0xdeadbeef);
  uint64_t rows_ai = 0, rows_sf = 0, rows_cf = 0;
  for (uint64_t s = 0; s < n; s++) {
    if (s % SL_TILE == 0) {
      const uint64_t k = s / SL_TILE;
      CHECK(ai.state[k] == ga.s && ai.rows[0][k] == rows_ai);
      CHECK(sf.state[k] == gs.s && sf.rows[0][k] == rows_sf && sf.rows[1][k] == rows_cf);
    }
    uint8_t ty[4];
    rows_ai += dint_pop::pick_types(ga, ty);
    const int m = dint_pop::pick_types(gs, ty);
    for (int i = 0; i < m; i++) {
      rows_sf++;
      gs.next();
      for (int st = 0; st < 3; st++)
        if (gs.next() % 2u != 0) {
          rows_cf++;
          gs.next();
        }
    }
  }
}

int main() {
  const std::vector<uint32_t> per = {0, 1, 4, 5, 8, 9, 41};
  placement_case(7, 0, 1, per, 40, -1);
  placement_case(7, 0, 1, per, 8, -1);
  placement_case(7, 0, 1, per, 40, 4);   // (bucket 4 holds 8 rows: rows 3 and 4 share a key across the entry boundary)
  placement_case(7, 0, 1, per, 8, 6);
  for (uint32_t index = 0; index < 3; index++) placement_case(21, index, 3, per, 40, 5);
  placement_case(20, 2, 3, {3, 0, 6, 13, 2, 9, 0}, 40, -1);  // (the last shard's last local bucket lies beyond the table)
  placement_case(1, 0, 1, {70}, 40, 0);
  jump_cases();
  generation_cases();
  if (bad) {
    printf("%d checks failed\n", bad);
    return 1;
  }
  printf("ok\n");
  return 0;
}
