// log_fold_main.cc -- the log fold's host form (dint_log_fold_host: dint_amd/csrc/k_fold.hip over log_fold.h) as a stand-alone
// program for a sanitizer run.  It reads the file `python tests/test_log_fold_host.py FILE` writes -- a few of that test's logs
// with the dumped rows they are folded against and the host form's flags, repair records and stats -- puts every array into a heap
// block of exactly its size, runs the host form and compares the return value, the flags, the records and the stats byte for
// byte.  The same rule header decides the device's bytes.  No device call.  Build and run (host code only; nothing of it is
// loaded into python):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tests/native/log_fold_main.cc dint_amd/csrc/k_fold.hip -o log_fold_main
//   ./log_fold_main FILE
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/dint_abi.h"
#include "../../include/dint_driver.h"

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
  uint64_t cases = 0;
  if (fread(&cases, 8, 1, f) != 1) return 2;
  int bad = 0;
  for (uint64_t i = 0; i < cases; i++) {
    uint32_t hd[2];  // workload, n_tables
    uint64_t hs[5], off[6], n = 0, n_rep = 0;
    if (fread(hd, 4, 2, f) != 2 || hd[1] < 1 || hd[1] > 5 || fread(hs, 8, 5, f) != 5 || fread(off, 8, 6, f) != 6) return 2;
    const uint64_t rows = off[hd[1]];
    block keys, vers, rec, flags, want_rep;
    if (!read_block(f, rows * 8, &keys) || !read_block(f, rows * 4, &vers) || fread(&n, 8, 1, f) != 1 || !read_block(f, n * 64, &rec) ||
        !read_block(f, n, &flags) || fread(&n_rep, 8, 1, f) != 1 || !read_block(f, n_rep * 64, &want_rep))
      return 2;
    dint_fold_stats want, got;
    if (fread(&want, sizeof want, 1, f) != 1) return 2;
    block out_flags = {(uint8_t *)malloc(n ? n : 1), (size_t)n}, out_rep = {(uint8_t *)malloc(n_rep ? n_rep * 64 : 1), (size_t)n_rep * 64};
    const int64_t rc = dint_log_fold_host(hd[0], hd[1], hs, off, (const uint64_t *)keys.p, (const uint32_t *)vers.p, rec.p, n, out_flags.p,
                                          out_rep.p, n_rep, &got);
    if (rc != (int64_t)n_rep || memcmp(out_flags.p, flags.p, n) != 0 || memcmp(out_rep.p, want_rep.p, n_rep * 64) != 0 ||
        memcmp(&got, &want, sizeof got) != 0) {
      printf("case %llu: rc %lld, expected %llu, or a flag, a record or a count differs\n", (unsigned long long)i, (long long)rc,
             (unsigned long long)n_rep);
      bad++;
    }
    // room for fewer repair records than there are: the first of them, and the count of all
    if (n_rep > 1) {
      block part = {(uint8_t *)malloc(64), 64};
      if (dint_log_fold_host(hd[0], hd[1], hs, off, (const uint64_t *)keys.p, (const uint32_t *)vers.p, rec.p, n, out_flags.p, part.p, 1,
                             &got) != 1 || got.repair_records != n_rep || memcmp(part.p, want_rep.p, 64) != 0)
        bad++;
      free(part.p);
    }
    if (dint_log_fold_host(hd[0], 0, hs, off, (const uint64_t *)keys.p, (const uint32_t *)vers.p, rec.p, n, out_flags.p, out_rep.p, n_rep,
                           &got) != DINT_EINVAL)
      bad++;
    block *all[] = {&keys, &vers, &rec, &flags, &want_rep, &out_flags, &out_rep};
    for (block *b : all) free(b->p);
  }
  fclose(f);
  printf("%llu cases, %d failures\n", (unsigned long long)cases, bad);
  return bad ? 1 : 0;
}
