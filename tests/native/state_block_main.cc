// state_block_main.cc -- the block sync's host forms (dint_state_block_digest_host / _rows_host / _diff_host: dint_amd/csrc/k_block.hip
// over state_block.h and state_sync.h, with the view check of k_verify.hip) as a stand-alone program for a sanitizer run.  It builds
// its own tables -- 300 buckets of 0 .. 6 rows, chains of three entries in the last bucket of block 0 and the first of block 1, a
// hole, a key held twice; the store's shape and smallbank's -- and a twin that differs in a known number of rows, puts every
// table, id list, row list and output into a heap block of exactly its size (row lists and outputs also at an odd address), and
// checks: the blocks of every size merge to the same table digest, the rows' count is the tables' distinct keys, a short cap
// gives the leading records, the diff of the twin has exactly the changes made, equal tables give none, and every refusal leaves
// its output as it was.  The same rule header guards the device's bounds.  No device call.  Build and run (host code only;
// nothing of it is loaded into python):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tests/native/state_block_main.cc dint_amd/csrc/k_block.hip dint_amd/csrc/k_verify.hip -o state_block_main
//   ./state_block_main
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "../../include/dint_abi.h"
#include "../../include/dint_driver.h"

static char g_err[512];
void dint_set_last_error(const char *msg) { snprintf(g_err, sizeof g_err, "%s", msg); }  // (engine.hip's, which is not linked here)

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
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      printf("line %d: %s (%s)\n", __LINE__, #cond, g_err);            \
      bad++;                                                           \
    }                                                                  \
  } while (0)

struct heap {  // exactly n bytes on the heap: one byte past it is the sanitizer's
  uint8_t *p;
  size_t n;
  explicit heap(size_t n_, int fill = 0) : p((uint8_t *)malloc(n_ ? n_ : 1)), n(n_) { memset(p, fill, n_ ? n_ : 1); }
  ~heap() { free(p); }
  heap(const heap &) = delete;
  bool all(int v) const {
    for (size_t i = 0; i < n; i++)
      if (p[i] != (uint8_t)v) return false;
    return true;
  }
};

struct table {
  static constexpr uint64_t N = 300;
  static constexpr uint32_t POOL = 128;
  uint32_t stride, vs;
  heap ent, nxt, ctl;
  uint32_t top = 0;
  uint64_t rows = 0, distinct = 0;
  table(uint32_t stride_) : stride(stride_), vs(stride_ == 256 ? 40 : 8), ent((N + POOL) * stride_), nxt(4 * POOL), ctl(DINT_VIEW_CTL_BYTES) {}
  uint8_t *entry(uint64_t e) { return ent.p + e * stride; }
  void put32(uint8_t *p, uint32_t v) { memcpy(p, &v, 4); }
  // row j of bucket b (chain order: the inline entry, then its overflow entries)
  void add(uint64_t b, uint32_t j, uint64_t key, uint32_t ver, uint8_t tag) {
    uint8_t *e = entry(b);
    if (j == 0) put32(e + 56, 1);  // head = the inline entry
    for (uint32_t x = 0; x < j / 4; x++) {
      uint32_t link;
      memcpy(&link, e + 52, 4);
      if (!link) {
        link = top++ + 2;
        put32(e + 52, link);
      }
      e = entry(N + link - 2);
    }
    const uint32_t s = j % 4;
    memcpy(e + 8 * s, &key, 8);
    put32(e + 32 + 4 * s, ver);
    e[48 + s] = 1;
    memset(e + 64 + vs * s, tag, vs);
    rows++;
  }
  void fill() {
    std::vector<uint32_t> have(N, 0), want(N);
    for (uint64_t b = 0; b < N; b++) want[b] = (uint32_t)(b % 7);
    want[63] = 10;
    want[64] = 9;
    uint64_t first64 = 0;
    for (uint64_t key = 1; key < 4000000; key++) {
      const uint64_t b = hash_key(key) % N;
      if (have[b] >= want[b]) continue;
      if (b == 64 && !first64) first64 = key;
      add(b, have[b]++, key, (uint32_t)key * 3u, (uint8_t)key);
      distinct++;
    }
    for (uint64_t b = 0; b < N; b++) CHECK(have[b] == want[b]);
    add(64, 9, first64, 77, 0x99);  // a second, shadowed row of bucket 64's first key
    entry(63)[48 + 2] = 0;          // a hole in bucket 63's chain
    rows--;
    distinct--;
    memcpy(ctl.p, &top, 4);
    CHECK(top <= POOL);
  }
  void view(dint_table_view &tv) {
    tv.entries = ent.p; tv.pool_next = (uint32_t *)nxt.p; tv.ctl = ctl.p;
    tv.n_local = N; tv.hash_size = N; tv.pool_cap = POOL; tv.stride = stride; tv.val_size = vs; tv.reserved = 0;
  }
};

static void run(uint32_t workload, uint32_t n_tables, uint32_t stride) {
  std::vector<table *> a, b;
  dint_tables_view va, vb;
  memset(&va, 0, sizeof va);
  va.workload = workload; va.n_tables = n_tables; va.shard_index = 0; va.shard_count = 1;
  vb = va;
  for (uint32_t t = 0; t < n_tables; t++) {
    a.push_back(new table(stride));
    b.push_back(new table(stride));
    a[t]->fill();
    b[t]->fill();
    a[t]->view(va.table[t]);
    b[t]->view(vb.table[t]);
  }
  // the twin: a value, a version, a row gone, a row of its own -- one of each per table
  uint64_t distinct = 0;
  for (uint32_t t = 0; t < n_tables; t++) {
    distinct += a[t]->distinct;
    b[t]->entry(5)[64] ^= 0x55;          // bucket 5, slot 0: the value
    b[t]->entry(6)[32] ^= 0x01;          // bucket 6, slot 0: the version alone
    b[t]->entry(12)[48] = 0;             // bucket 12, slot 0: gone
    uint64_t key = 5000000;
    while (hash_key(key) % table::N != 7) key++;
    b[t]->add(7, 0, key, 1, 2);          // bucket 7 (empty in a): a row only the twin has
  }
  // digests: every block size merges to the same table digests
  uint64_t merged[3][5][3];
  memset(merged, 0, sizeof merged);
  const uint64_t sizes[3] = {64, 256, 1u << 20};
  for (int k = 0; k < 3; k++) {
    dint_block_stats st;
    const int64_t n = dint_state_block_digest_host(&va, sizes[k], nullptr, 0, &st);
    CHECK(n == (int64_t)n_tables * (k == 0 ? 5 : k == 1 ? 2 : 1) && st.n_blocks == n && st.total == (uint64_t)n);
    heap out((size_t)n * sizeof(dint_block_digest), 0xEE);
    CHECK(dint_state_block_digest_host(&va, sizes[k], (dint_block_digest *)out.p, (uint64_t)n, &st) == n);
    heap small((size_t)(n - 1) * sizeof(dint_block_digest), 0xEE);
    CHECK(dint_state_block_digest_host(&va, sizes[k], (dint_block_digest *)small.p, (uint64_t)n - 1, &st) == DINT_EINVAL && small.all(0xEE));
    uint32_t id = 0;
    for (uint32_t t = 0; t < n_tables; t++)
      for (uint32_t j = 0; j < st.blocks[t]; j++, id++) {
        const dint_block_digest *d = (const dint_block_digest *)out.p + id;
        merged[k][t][0] += d->rows; merged[k][t][1] += d->sum; merged[k][t][2] ^= d->xr;
        CHECK(d->reserved == 0);
      }
  }
  for (uint32_t t = 0; t < n_tables; t++) {
    CHECK(merged[0][t][0] == a[t]->rows);
    CHECK(memcmp(merged[0][t], merged[1][t], 24) == 0 && memcmp(merged[0][t], merged[2][t], 24) == 0);
  }
  // rows and the diff, at every block size; the lists at an odd address
  for (int k = 0; k < 3; k++) {
    const uint32_t n_ids = n_tables * (k == 0 ? 5 : k == 1 ? 2 : 1);
    heap ids((size_t)n_ids * 4);
    for (uint32_t i = 0; i < n_ids; i++) ((uint32_t *)ids.p)[i] = i;
    dint_block_stats st;
    CHECK(dint_state_block_rows_host(&va, sizes[k], (const uint32_t *)ids.p, n_ids, nullptr, 0, &st) == 0 && st.total == distinct);
    heap rows(1 + (size_t)st.total * 64, 0xEE);
    CHECK(dint_state_block_rows_host(&va, sizes[k], (const uint32_t *)ids.p, n_ids, rows.p + 1, st.total, &st) == (int64_t)distinct);
    std::set<uint64_t> keys;
    for (uint64_t i = 0; i < distinct; i++) {
      uint64_t key;
      memcpy(&key, rows.p + 1 + i * 64, 8);
      keys.insert(key ^ ((uint64_t)rows.p[1 + i * 64 + 53] << 60));
      CHECK(rows.p[1 + i * 64 + 52] == 0);
    }
    CHECK(keys.size() == distinct && rows.p[0] == 0xEE);
    heap lead(1 + 10 * 64, 0xEE);
    CHECK(dint_state_block_rows_host(&va, sizes[k], (const uint32_t *)ids.p, n_ids, lead.p + 1, 10, &st) == 10 && st.total == distinct);
    CHECK(memcmp(lead.p + 1, rows.p + 1, 640) == 0);
    // the twin's diff: per table one value, one version, one row to insert, one to delete
    dint_diff_stats ds;
    CHECK(dint_state_block_diff_host(&vb, sizes[k], (const uint32_t *)ids.p, n_ids, rows.p + 1, distinct, nullptr, 0, &ds) == 0);
    CHECK(ds.total == 4 * n_tables && ds.only_a == n_tables && ds.only_b == n_tables && ds.val_differs == n_tables && ds.ver_only == n_tables);
    heap rec(1 + (size_t)ds.total * 64, 0xEE);
    CHECK(dint_state_block_diff_host(&vb, sizes[k], (const uint32_t *)ids.p, n_ids, rows.p + 1, distinct, rec.p + 1, ds.total, &ds) == (int64_t)ds.total);
    heap one(64, 0xEE);
    CHECK(dint_state_block_diff_host(&vb, sizes[k], (const uint32_t *)ids.p, n_ids, rows.p + 1, distinct, one.p, 1, &ds) == 1 && memcmp(one.p, rec.p + 1, 64) == 0);
    CHECK(dint_state_block_diff_host(&va, sizes[k], (const uint32_t *)ids.p, n_ids, rows.p + 1, distinct, one.p, 1, &ds) == 0 && ds.total == 0);
    // refusals: the output stays as it was
    heap out(256 * 64, 0xEE);
    heap rev((size_t)distinct * 64);
    for (uint64_t i = 0; i < distinct; i++) memcpy(rev.p + i * 64, rows.p + 1 + (distinct - 1 - i) * 64, 64);
    CHECK(dint_state_block_diff_host(&vb, sizes[k], (const uint32_t *)ids.p, n_ids, rev.p, distinct, out.p, 256, &ds) == DINT_EINVAL && out.all(0xEE));
    if (n_ids > 1) {
      CHECK(dint_state_block_diff_host(&vb, sizes[k], (const uint32_t *)ids.p + 1, n_ids - 1, rows.p + 1, distinct, out.p, 256, &ds) == DINT_EINVAL);
      heap down((size_t)n_ids * 4);
      for (uint32_t i = 0; i < n_ids; i++) ((uint32_t *)down.p)[i] = n_ids - 1 - i;
      CHECK(dint_state_block_rows_host(&va, sizes[k], (const uint32_t *)down.p, n_ids, out.p, 256, &st) == DINT_EINVAL);
      ((uint32_t *)down.p)[0] = ((uint32_t *)down.p)[1] = 0;
      CHECK(dint_state_block_rows_host(&va, sizes[k], (const uint32_t *)down.p, 2, out.p, 256, &st) == DINT_EINVAL);
    }
    uint32_t beyond = n_ids;
    CHECK(dint_state_block_rows_host(&va, sizes[k], &beyond, 1, out.p, 256, &st) == DINT_EINVAL);
    CHECK(dint_state_block_diff_host(&vb, sizes[k], &beyond, 1, rows.p + 1, 1, out.p, 256, &ds) == DINT_EINVAL);
    rev.p[53] = 7;  // table 7
    CHECK(dint_state_block_diff_host(&vb, sizes[k], (const uint32_t *)ids.p, n_ids, rev.p, 1, out.p, 256, &ds) == DINT_EINVAL);
    CHECK(out.all(0xEE));
  }
  heap out(64 * 64, 0xEE);
  uint32_t zero = 0;
  for (uint64_t B : {96ull, 32ull, 0ull, 1ull << 21}) {
    CHECK(dint_state_block_digest_host(&va, B, (dint_block_digest *)out.p, 64, nullptr) == DINT_EINVAL);
    CHECK(dint_state_block_rows_host(&va, B, &zero, 1, out.p, 64, nullptr) == DINT_EINVAL);
    CHECK(dint_state_block_diff_host(&vb, B, &zero, 1, out.p, 0, out.p, 64, nullptr) == DINT_EINVAL);
  }
  CHECK(out.all(0xEE));
  for (table *t : a) delete t;
  for (table *t : b) delete t;
}

int main() {
  run(DINT_WL_STORE, 1, 256);
  run(DINT_WL_SMALLBANK, 2, 128);
  printf("%d failures\n", bad);
  return bad ? 1 : 0;
}
