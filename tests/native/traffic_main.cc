// traffic_main.cc -- the traffic report's host form (dint_traffic_report_host: dint_amd/csrc/k_traffic.hip over traffic_report.h) as a
// stand-alone program for a sanitizer run.  For the five keyed workloads it builds batches and reply arrays, puts every array --
// requests, replies, the report, the two lists -- into a heap block of exactly its size (requests and replies also at an odd
// address), asks for more list entries than there are distinct keys, and checks what this file counts itself: requests, bad tables,
// distinct (table, key) pairs with a std::set, the per-key request counts of the by-requests list and its order, the type
// histograms' sums.  Every refusal must leave its outputs as they were.  No device call.  Build and run (host code only; nothing of
// it is loaded into python):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tests/native/traffic_main.cc dint_amd/csrc/k_traffic.hip -o traffic_main
//   ./traffic_main
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "../../include/dint_abi.h"
#include "../../include/dint_driver.h"

static char g_err[512];
void dint_set_last_error(const char *msg) { snprintf(g_err, sizeof g_err, "%s", msg); }  // (engine.hip's, which is not linked here)

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

static uint64_t rnd_state = 99;
static uint64_t rnd() {
  rnd_state = rnd_state * 6364136223846793005ULL + 1442695040888963407ULL;
  return rnd_state >> 11;
}

struct shape {
  uint32_t wl, msg, type_at, table_at, key_at, key_bytes, n_tables;
};
static const shape SHAPES[] = {{DINT_WL_FASST, 9, 0, 99, 1, 4, 1}, {DINT_WL_2PL, 6, 0, 99, 1, 4, 1}, {DINT_WL_STORE, 53, 0, 99, 1, 8, 1},
                               {DINT_WL_TATP, 55, 1, 2, 3, 8, 5}, {DINT_WL_SMALLBANK, 23, 1, 2, 3, 8, 2}};

static void fill(const shape &s, uint8_t *m, uint64_t n, uint64_t key_space) {
  for (uint64_t i = 0; i < n; i++) {
    uint8_t *r = m + i * s.msg;
    for (uint32_t k = 0; k < s.msg; k++) r[k] = (uint8_t)rnd();
    r[s.type_at] = (uint8_t)(rnd() % 30);
    if (s.wl == DINT_WL_2PL) r[5] = (uint8_t)(rnd() % 3);
    if (s.table_at != 99) r[s.table_at] = (uint8_t)(rnd() % (s.n_tables + 1));  // (one in n_tables + 1: a table the workload has not)
    uint64_t key = rnd() % key_space;
    if (i % 17 == 0) key = s.key_bytes == 4 ? 0xFFFFFFFFull : ~0ull;
    if (i % 19 == 0) key = 0;
    memcpy(r + s.key_at, &key, s.key_bytes);
  }
}

static void run(const shape &s, uint64_t n, uint64_t key_space, uint32_t top_k, size_t odd, bool with_replies) {
  heap req(odd + n * s.msg), rep(odd + n * s.msg), out(sizeof(struct dint_traffic_report), 0xEE), a((size_t)top_k * sizeof(dint_traffic_key), 0xEE),
      b((size_t)top_k * sizeof(dint_traffic_key), 0xEE);
  fill(s, req.p + odd, n, key_space);
  fill(s, rep.p + odd, n, key_space);
  const int rc = dint_traffic_report_host(s.wl, 16, 64, 0, n ? req.p + odd : nullptr, with_replies ? rep.p + odd : nullptr, n, top_k,
                                          (struct dint_traffic_report *)out.p, top_k ? (dint_traffic_key *)a.p : nullptr, top_k ? (dint_traffic_key *)b.p : nullptr);
  CHECK(rc == 0);
  if (rc) return;
  struct dint_traffic_report r;
  memcpy(&r, out.p, sizeof r);
  uint64_t bad_table = 0, in_hist = 0, in_rep = 0;
  for (uint64_t i = 0; i < n; i++)
    if (s.table_at != 99 && req.p[odd + i * s.msg + s.table_at] >= s.n_tables) bad_table++;
  for (int t = 0; t < 5; t++)
    for (int y = 0; y < 32; y++) in_hist += r.req_types[t][y], in_rep += r.rep_types[t][y];
  CHECK(r.n == n && r.bad_table == bad_table && in_hist == n - bad_table && in_rep == (with_replies ? n - bad_table : 0));
  CHECK(r.keyed + r.log_requests + r.bad_table == n && r.reads + r.locks + r.unlocks + r.writes + r.others == r.keyed);
  CHECK(r.temp_bytes == 0 && r.distinct_units <= r.distinct_keys && r.distinct_keys <= r.keyed);
  if (!with_replies) CHECK(r.rejects == 0 && r.misses == 0 && r.n_by_rejects == 0 && r.shared_unit_rejects == 0 && r.shared_slot_rejects == 0);
  // the by-requests list: top_k is larger than the distinct keys in the small shapes, so it is ALL of them
  const dint_traffic_key *l = (const dint_traffic_key *)a.p;
  CHECK(r.n_by_requests == (r.distinct_keys < top_k ? r.distinct_keys : top_k));
  uint64_t sum = 0;
  std::set<std::pair<uint32_t, uint64_t>> seen;
  for (uint64_t k = 0; k < r.n_by_requests; k++) {
    sum += l[k].requests;
    CHECK(seen.insert({l[k].table, l[k].key}).second && l[k].table < s.n_tables && l[k].first_index < n && l[k].reserved == 0);
    if (k) CHECK(l[k - 1].requests > l[k].requests || (l[k - 1].requests == l[k].requests && (l[k - 1].table < l[k].table ||
                 (l[k - 1].table == l[k].table && l[k - 1].key < l[k].key))));
    uint64_t key = 0;
    memcpy(&key, req.p + odd + (size_t)l[k].first_index * s.msg + s.key_at, s.key_bytes);
    CHECK(key == l[k].key);
  }
  if (r.distinct_keys <= top_k) CHECK(sum == r.keyed);
  for (size_t k = r.n_by_requests * sizeof(dint_traffic_key); k < a.n; k++) CHECK(a.p[k] == 0xEE);
  for (size_t k = r.n_by_rejects * sizeof(dint_traffic_key); k < b.n; k++) CHECK(b.p[k] == 0xEE);
}

static void refusals() {
  const shape &s = SHAPES[3];
  const uint64_t n = 40;
  heap req(n * s.msg), rep(n * s.msg), out(sizeof(struct dint_traffic_report), 0xEE), a(4 * sizeof(dint_traffic_key), 0xEE), b(4 * sizeof(dint_traffic_key), 0xEE);
  fill(s, req.p, n, 10);
  struct dint_traffic_report *o = (struct dint_traffic_report *)out.p;
  dint_traffic_key *la = (dint_traffic_key *)a.p, *lb = (dint_traffic_key *)b.p;
  CHECK(dint_traffic_report_host(DINT_WL_LOG, 16, 64, 0, req.p, rep.p, n, 4, o, la, lb) == DINT_ESTATE);
  CHECK(dint_traffic_report_host(77, 16, 64, 0, req.p, rep.p, n, 4, o, la, lb) == DINT_EINVAL);
  CHECK(dint_traffic_report_host(s.wl, 16, 64, 0, req.p, req.p, n, 4, o, la, lb) == DINT_EINVAL);  // replies == requests
  CHECK(dint_traffic_report_host(s.wl, 16, 64, 0, nullptr, rep.p, n, 4, o, la, lb) == DINT_EINVAL);
  CHECK(dint_traffic_report_host(s.wl, 16, 64, 0, req.p, rep.p, n, 4, nullptr, la, lb) == DINT_EINVAL);
  CHECK(dint_traffic_report_host(s.wl, 16, 64, 0, req.p, rep.p, n, 4, o, nullptr, lb) == DINT_EINVAL);
  CHECK(dint_traffic_report_host(s.wl, 16, 64, 0, req.p, rep.p, n, 4, o, la, nullptr) == DINT_EINVAL);
  CHECK(dint_traffic_report_host(s.wl, 16, 64, 0, req.p, rep.p, n, 4097, o, la, lb) == DINT_EINVAL);
  CHECK(dint_traffic_report_host(s.wl, 16, 64, 0, req.p, rep.p, (1ull << 24) + 1, 4, o, la, lb) == DINT_EINVAL);  // (refused before a byte is read)
  CHECK(out.all(0xEE) && a.all(0xEE) && b.all(0xEE));
}

int main() {
  for (const shape &s : SHAPES) {
    run(s, 0, 10, 8, 0, true);
    run(s, 1, 10, 8, 1, true);
    run(s, 300, 12, 4096, 1, true);    // a dozen keys per table: top_k far above the distinct keys
    run(s, 300, 12, 4096, 3, false);
    run(s, 5000, 1ull << 40, 16, 7, true);
    run(s, 2000, 40, 0, 1, true);      // no lists
  }
  refusals();
  printf("%d failures\n", bad);
  return bad ? 1 : 0;
}
