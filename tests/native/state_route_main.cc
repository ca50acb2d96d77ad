// state_route_main.cc -- the record routing's host form (dint_records_route_host: dint_amd/csrc/k_rroute.hip over state_route.h) as a
// stand-alone program for a sanitizer run.  It builds lists of canonical 64-byte records over every table of a workload, puts every
// list, output and offset array into a heap block of exactly its size (lists and outputs also at an odd address), and checks: the
// offsets count the homes this file computes itself, every shard's piece holds exactly the records of that home in their input
// order, 255 shards with a handful of records, one key for every record, no record at all, and that every refusal leaves its
// output as it was.  The same rule header guards the device's bounds.  No device call.  Build and run (host code only; nothing of
// it is loaded into python):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tests/native/state_route_main.cc dint_amd/csrc/k_rroute.hip -o state_route_main
//   ./state_route_main
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static uint64_t rnd_state = 12345;
static uint64_t rnd() {
  rnd_state = rnd_state * 6364136223846793005ULL + 1442695040888963407ULL;
  return rnd_state >> 11;
}

// the workload's bucket counts (store/udp/server.cc:112-114, tatp/udp/server_shard.cc:75-79, smallbank/udp/server_shard.cc:75-76)
static std::vector<uint64_t> sizes(uint32_t wl, uint64_t n) {
  if (wl == DINT_WL_STORE) return {n * 18 / 4};
  if (wl == DINT_WL_TATP) return {n * 3 / 2 / 4, n * 3 / 2 / 4, n * 15 / 4 / 4, n * 15 / 4 / 4, n * 45 / 8 / 4};
  return {n * 3 / 2 / 4, n * 3 / 2 / 4};
}

static void fill(uint8_t *rec, uint64_t n, uint32_t n_tables, bool one_key) {
  for (uint64_t i = 0; i < n; i++) {
    uint8_t *r = rec + i * 64;
    for (int k = 0; k < 64; k++) r[k] = (uint8_t)rnd();
    const uint64_t key = one_key ? 77 : rnd() % (1ull << 44) + 1;
    memcpy(r, &key, 8);
    r[53] = one_key ? 0 : (uint8_t)(rnd() % n_tables);
  }
}

static void run(uint32_t wl, uint64_t n_rows, uint32_t H, uint64_t n, bool one_key, size_t odd) {
  const std::vector<uint64_t> hs = sizes(wl, n_rows ? n_rows : 7000000);  // (0: tatp's own size, tatp/udp/tatp.h:28)
  heap rec(odd + n * 64), out(odd + n * 64, 0xEE), off((size_t)(H + 1) * 8, 0xEE);
  fill(rec.p + odd, n, (uint32_t)hs.size(), one_key);
  CHECK(dint_records_route_host(wl, n_rows, H, n ? rec.p + odd : nullptr, n, n ? out.p + odd : nullptr, (uint64_t *)off.p) == (int64_t)n);
  std::vector<uint64_t> at(H + 1, 0);
  std::vector<uint32_t> home(n);
  for (uint64_t i = 0; i < n; i++) {
    uint64_t key;
    memcpy(&key, rec.p + odd + i * 64, 8);
    home[i] = (uint32_t)((hash_key(key) % hs[rec.p[odd + i * 64 + 53]]) % H);
    at[home[i] + 1]++;
  }
  for (uint32_t h = 0; h < H; h++) at[h + 1] += at[h];
  CHECK(memcmp(off.p, at.data(), off.n) == 0);
  for (uint64_t i = 0; i < n; i++) CHECK(memcmp(out.p + odd + at[home[i]]++ * 64, rec.p + odd + i * 64, 64) == 0);
  for (size_t k = 0; k < odd; k++) CHECK(out.p[k] == 0xEE);
}

static void refusals() {
  const uint64_t n = 50;
  heap rec(n * 64), out(n * 64, 0xEE), off(4 * 8, 0xEE);
  fill(rec.p, n, 5, false);
  uint64_t *o = (uint64_t *)off.p;
  CHECK(dint_records_route_host(DINT_WL_TATP, 300, 0, rec.p, n, out.p, o) == DINT_EINVAL);
  CHECK(dint_records_route_host(DINT_WL_TATP, 300, 256, rec.p, n, out.p, o) == DINT_EINVAL);
  CHECK(dint_records_route_host(DINT_WL_TATP, 300, 3, rec.p, n, out.p, nullptr) == DINT_EINVAL);
  CHECK(dint_records_route_host(DINT_WL_TATP, 300, 3, nullptr, n, out.p, o) == DINT_EINVAL);
  CHECK(dint_records_route_host(DINT_WL_TATP, 300, 3, rec.p, n, nullptr, o) == DINT_EINVAL);
  CHECK(dint_records_route_host(DINT_WL_FASST, 300, 3, rec.p, n, out.p, o) == DINT_ESTATE);
  CHECK(dint_records_route_host(DINT_WL_LOG, 300, 3, rec.p, n, out.p, o) == DINT_ESTATE);
  CHECK(dint_records_route_host(DINT_WL_TATP, 300, 3, rec.p, n, rec.p + 64, o) == DINT_EINVAL);  // overlapping
  rec.p[(n - 1) * 64 + 53] = 5;  // the last record: a table tatp has not
  CHECK(dint_records_route_host(DINT_WL_TATP, 300, 3, rec.p, n, out.p, o) == DINT_EINVAL && strstr(g_err, "record 49 "));
  rec.p[7 * 64 + 53] = 255;
  CHECK(dint_records_route_host(DINT_WL_TATP, 300, 3, rec.p, n, out.p, o) == DINT_EINVAL && strstr(g_err, "record 7 "));
  rec.p[7 * 64 + 53] = 1;
  rec.p[(n - 1) * 64 + 53] = 2;
  CHECK(dint_records_route_host(DINT_WL_SMALLBANK, 1000, 3, rec.p, n, out.p, o) == DINT_EINVAL);  // smallbank has two tables
  CHECK(out.all(0xEE) && off.all(0xEE));
}

int main() {
  const uint32_t Hs[] = {1, 2, 3, 5, 64, 255};
  const struct { uint32_t wl; uint64_t n_rows; } shapes[] = {{DINT_WL_TATP, 300}, {DINT_WL_SMALLBANK, 1000}, {DINT_WL_STORE, 1000}};
  for (const auto &s : shapes)
    for (uint32_t H : Hs) {
      run(s.wl, s.n_rows, H, 0, false, 0);
      run(s.wl, s.n_rows, H, 1, false, 1);
      run(s.wl, s.n_rows, H, 513, true, 0);
      run(s.wl, s.n_rows, H, 1500, false, 3);
    }
  run(DINT_WL_TATP, 0, 255, 40, false, 0);  // the reference's own size; most shards empty
  refusals();
  printf("%d failures\n", bad);
  return bad ? 1 : 0;
}
