// state_compact_main.cc -- the table compaction's host form (dint_state_compact_view_host: dint_amd/csrc/k_compact.hip over
// state_compact.h, with the census of k_verify.hip) as a stand-alone program for a sanitizer run.  It reads the file
// `python tests/test_state_compact_host.py FILE` writes -- every view of that test, the dry runs and the damaged ones included, with
// the numpy form's reports and the bytes a compaction must leave -- puts every array into a heap block of exactly its size, runs
// the host form and compares the return value, the reports word for word and the bytes afterwards.  The same rule header guards
// the device's bounds.  No device call.  Build and run (host code only; nothing of it is loaded into python):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tests/native/state_compact_main.cc dint_amd/csrc/k_compact.hip dint_amd/csrc/k_verify.hip -o state_compact_main
//   ./state_compact_main FILE
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/dint_abi.h"
#include "../../include/dint_driver.h"

static char g_err[512];
void dint_set_last_error(const char *msg) { snprintf(g_err, sizeof g_err, "%s", msg); }  // (engine.hip's, which is not linked here)

struct block {  // exactly n bytes on the heap, aligned as malloc aligns: one byte past it is the sanitizer's
  uint8_t *p;
  size_t n;
};
static bool read_block(FILE *f, size_t n, block *b) {
  b->n = n;
  b->p = (uint8_t *)malloc(n ? n : 1);
  return fread(b->p, 1, n, f) == n;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t n = 0;
  if (fread(&n, 8, 1, f) != 1) return 2;
  int bad = 0;
  for (uint64_t i = 0; i < n; i++) {
    int32_t hd[6];  // workload, n_tables, shard_index, shard_count, flags, rc
    if (fread(hd, 4, 6, f) != 6 || hd[1] < 1 || hd[1] > 5) return 2;
    const uint32_t tables = (uint32_t)hd[1];
    dint_tables_view v;
    memset(&v, 0, sizeof v);
    v.workload = (uint32_t)hd[0]; v.n_tables = tables; v.shard_index = (uint32_t)hd[2]; v.shard_count = (uint32_t)hd[3];
    block ent[5], nxt[5], ctl[5];
    for (uint32_t t = 0; t < tables; t++) {
      uint64_t g[5];  // n_local, hash_size, pool_cap, stride, val_size
      if (fread(g, 8, 5, f) != 5) return 2;
      if (!read_block(f, (size_t)((g[0] + g[2]) * g[3]), &ent[t]) || !read_block(f, (size_t)(4 * g[2]), &nxt[t]) ||
          !read_block(f, DINT_VIEW_CTL_BYTES, &ctl[t]))
        return 2;
      dint_table_view &tv = v.table[t];
      tv.entries = ent[t].p; tv.pool_next = (uint32_t *)nxt[t].p; tv.ctl = ctl[t].p;
      tv.n_local = g[0]; tv.hash_size = g[1]; tv.pool_cap = (uint32_t)g[2]; tv.stride = (uint32_t)g[3]; tv.val_size = (uint32_t)g[4];
    }
    std::vector<uint64_t> want((size_t)tables * 64);
    if (fread(want.data(), 8, want.size(), f) != want.size()) return 2;
    std::vector<dint_table_compact> out(tables);
    const int rc = dint_state_compact_view_host(&v, out.data(), tables, (uint32_t)hd[4]);
    if (rc != hd[5] || memcmp(out.data(), want.data(), want.size() * 8) != 0) {
      printf("view %llu: rc %d, expected %d (%s), or a word differs\n", (unsigned long long)i, rc, hd[5], g_err);
      bad++;
    }
    for (uint32_t t = 0; t < tables; t++) {
      block *have[3] = {&ent[t], &nxt[t], &ctl[t]};
      for (block *b : have) {
        std::vector<uint8_t> after(b->n);
        if (fread(after.data(), 1, b->n, f) != b->n) return 2;
        if (memcmp(after.data(), b->p, b->n) != 0) {
          printf("view %llu table %u: the bytes afterwards differ\n", (unsigned long long)i, t);
          bad++;
        }
      }
    }
    if (dint_state_compact_view_host(&v, out.data(), tables - 1, 0) != DINT_EINVAL) bad++;
    for (uint32_t t = 0; t < tables; t++) { free(ent[t].p); free(nxt[t].p); free(ctl[t].p); }
  }
  fclose(f);
  printf("%llu views, %d failures\n", (unsigned long long)n, bad);
  return bad ? 1 : 0;
}
