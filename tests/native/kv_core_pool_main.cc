// Stand-alone driver of the host build of the table layout (dint_amd/csrc/dint_kv_core.h through kv_core_host.cc) with overflow
// pools the op stream overruns, against the oracle's chained kvs (oracle/dint_oracle.c) with the refused inserts skipped: the
// same walk as tests/test_kv_core_host.py test_overrun_pool_refuses_and_stays_exact, with a main of its own so that it can be
// built with -fsanitize=address,undefined and run as it is.  TEST TOOLING ONLY.
//   gcc -c -O1 -g -fsanitize=address,undefined oracle/dint_oracle.c -o dint_oracle.o
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Wno-unknown-pragmas tests/native/kv_core_pool_main.cc dint_oracle.o -o kv_core_pool
#include <stdio.h>

#include <vector>

#include "kv_core_host.cc"
extern "C" {
#include "../../oracle/dint_oracle.h"
}

static uint64_t rng_state;
static uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

static int same_dump(kvh *h, orc_kvs *o, uint32_t vs) {
  const uint64_t n = kvh_dump(h, nullptr, nullptr, nullptr, 0);
  if (n != orc_kvs_count(o)) return 0;
  std::vector<uint64_t> ka(n + 1), kb(n + 1);
  std::vector<uint32_t> va(n + 1), vb(n + 1);
  std::vector<uint8_t> la((n + 1) * vs), lb((n + 1) * vs);
  kvh_dump(h, ka.data(), va.data(), la.data(), n);
  orc_kvs_dump(o, kb.data(), vb.data(), lb.data(), n);
  return !memcmp(ka.data(), kb.data(), n * 8) && !memcmp(va.data(), vb.data(), n * 4) && !memcmp(la.data(), lb.data(), n * vs);
}

static int run(uint32_t vs, uint32_t nb, uint32_t nkeys, uint32_t pool, uint32_t nops, uint64_t seed, int dups) {
  rng_state = seed * 0x9E3779B97F4A7C15ull + 1;
  kvh *h = kvh_create(nb, pool, vs);
  orc_kvs *o = orc_kvs_create(nb, vs);
  std::vector<uint64_t> keys(nkeys);
  std::vector<int> live(nkeys, 0);
  for (auto &k : keys) k = (rnd() >> 2) | 1;
  uint32_t refused = 0, stored = 0;
  int bad = 0;
  for (uint32_t step = 0; step < nops && !bad; step++) {
    const uint32_t ki = (uint32_t)(rnd() % nkeys), op = (uint32_t)(rnd() % 10);
    const uint64_t k = keys[ki], b = orc_fasthash64(&k, 8, 0xDEADBEEF) % nb;
    uint8_t val[40], gv[40], ov[40];
    for (uint32_t i = 0; i < vs; i++) val[i] = (uint8_t)rnd();
    if (op < 3) {
      uint32_t gver = 0, over = 0;
      const int ra = kvh_get(h, b, k, gv, &gver), rb = orc_kvs_get(o, k, ov, &over);
      bad |= (ra != 0) != (rb != 0) || (!ra && (memcmp(gv, ov, vs) || gver != over));
    } else if (op < 5) {
      bad |= kvh_set(h, b, k, val) != orc_kvs_set(o, k, val);
    } else if (op < 8) {
      if (!dups && live[ki] > 0) continue;
      const uint32_t top = kvh_pool_top(h), fr = kvh_listed(h, 0);
      if (kvh_insert(h, b, k, val, 0) == 0) {
        orc_kvs_insert(o, k, val);
        live[ki]++; stored++;
      } else {  // refused: only with nothing left to hand out, and nothing was stored (the oracle skips it)
        bad |= top != pool || fr != 0;
        refused++;
      }
      bad |= kvh_pool_top(h) > pool || (refused && kvh_pool_top(h) != pool);  // the clamp: the counter stays at pool_cap
    } else {
      const int rc = orc_kvs_delete(o, k);
      bad |= kvh_delete(h, b, k) != rc;
      if (rc == 0) live[ki]--;
    }
    if (step % 97 == 0) kvh_rotate(h);
    if (step % 500 == 0) bad |= !same_dump(h, o, vs);
    if (bad) fprintf(stderr, "mismatch at step %u (pool %u, seed %llu)\n", step, pool, (unsigned long long)seed);
  }
  bad |= !same_dump(h, o, vs);
  printf("vs %u buckets %u keys %u pool %u: %u inserts stored, %u refused%s\n", vs, nb, nkeys, pool, stored, refused, bad ? "  MISMATCH" : "");
  if (!refused) { fprintf(stderr, "the op stream never overran the pool\n"); bad = 1; }
  orc_kvs_destroy(o);
  kvh_destroy(h);
  return bad;
}

int main() {
  int bad = 0;
  bad |= run(40, 1, 40, 2, 6000, 1, 0);
  bad |= run(40, 3, 90, 5, 9000, 2, 0);
  bad |= run(8, 2, 120, 9, 9000, 3, 0);
  bad |= run(40, 2, 24, 5, 6000, 4, 1);
  bad |= run(8, 1, 12, 9, 5000, 5, 1);
  bad |= run(40, 7, 400, 9, 20000, 6, 0);
  printf(bad ? "FAILED\n" : "ok\n");
  return bad;
}
