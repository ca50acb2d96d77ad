// state_locks_main.cc -- the held locks' host forms (dint_state_locks_image_host / dint_state_unlock_check_host:
// dint_amd/csrc/k_locks_state.hip over state_locks.h, behind dint_state_image_check_host of k_image.hip) as a stand-alone program
// for a sanitizer run.  It reads the file `python tests/test_state_locks_host.py FILE` writes -- the hand-built images of that test
// with the numpy form's lists and statistics, then the list-check cases with the index each must be refused at -- feeds every
// image and list to the host forms from heap blocks of exactly their size, the records at an odd address, and compares byte for
// byte; then the same image truncated, with a cap one short, and with its links bent, which must be refused or stay inside the
// image.  No device call.  Build and run (host code only; nothing of it is loaded into python):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tests/native/state_locks_main.cc dint_amd/csrc/k_locks_state.hip dint_amd/csrc/k_image.hip -o state_locks_main
//   ./state_locks_main FILE
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/dint_abi.h"
#include "../../include/dint_driver.h"

static char g_err[512];
void dint_set_last_error(const char *msg) { snprintf(g_err, sizeof g_err, "%s", msg); }  // (engine.hip's, which is not linked here)

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t n = 0;
  if (fread(&n, 8, 1, f) != 1) return 2;
  int bad = 0;
  for (uint64_t i = 0; i < n; i++) {
    uint64_t hd[2];
    if (fread(hd, 8, 2, f) != 2) return 2;
    const uint64_t bytes = hd[0], recs = hd[1], padded = (bytes + 7) / 8 * 8;
    std::vector<uint8_t> img(padded), want(recs * 32);
    uint64_t st[10];
    if (fread(img.data(), 1, padded, f) != padded || fread(want.data(), 1, want.size(), f) != want.size() || fread(st, 8, 10, f) != 10) return 2;
    img.resize(bytes);
    img.shrink_to_fit();  // the sanitizer sees a read one byte past the image
    std::vector<uint8_t> out(recs * 32 + 1);  // ... and a write past the cap records; the records start at an odd address
    dint_lock_stats s;
    const int64_t rc = dint_state_locks_image_host(img.data(), bytes, (dint_lock_record *)(out.data() + 1), recs, &s);
    if (rc != (int64_t)recs || (recs && memcmp(out.data() + 1, want.data(), want.size()) != 0) || memcmp(&s, st, sizeof st) != 0) {
      printf("image %llu: rc %lld (%s), or a byte differs\n", (unsigned long long)i, (long long)rc, g_err);
      bad++;
    }
    if (recs) {  // a cap one short: the first records, the same total
      std::vector<uint8_t> cut((recs - 1) * 32 + 1);
      const int64_t rs = dint_state_locks_image_host(img.data(), bytes, (dint_lock_record *)(cut.data() + 1), recs - 1, &s);
      if (rs != (int64_t)recs - 1 || s.total != recs || memcmp(cut.data() + 1, want.data(), (recs - 1) * 32) != 0) bad++;
    }
    if (dint_state_locks_image_host(img.data(), bytes, nullptr, 0, &s) != 0 || s.total != recs) bad++;
    if (bytes > 400) {
      if (dint_state_locks_image_host(img.data(), bytes - 16, (dint_lock_record *)(out.data() + 1), recs, &s) != DINT_EINVAL) bad++;
      std::vector<uint8_t> bent(img);  // bytes 52..59 of every 64 behind the header overwritten: links, ids and values far outside
      for (uint64_t at = 320; at + 64 <= bytes; at += 64) memset(bent.data() + at + 52, 0xEE, 8);
      std::vector<uint8_t> any(4 * (bytes / 16) * 32 + 32);
      const int64_t rb = dint_state_locks_image_host(bent.data(), bytes, (dint_lock_record *)any.data(), any.size() / 32, &s);
      if (rb != DINT_EINVAL && rb < 0) bad++;  // (refused by the check, or still an image: either way nothing outside it is read)
    }
  }
  uint64_t lists = 0;
  if (fread(&lists, 8, 1, f) != 1) return 2;
  for (uint64_t i = 0; i < lists; i++) {
    uint32_t workload;
    dint_lock_geometry g;
    uint64_t hd[2];
    static_assert(sizeof g == 56, "the fixture's geometry");
    if (fread(&workload, 4, 1, f) != 1 || fread(&g, sizeof g, 1, f) != 1 || fread(hd, 8, 2, f) != 2) return 2;
    std::vector<uint8_t> r(hd[0] * 32 + 1);
    if (hd[0] && fread(r.data() + 1, 32, hd[0], f) != hd[0]) return 2;
    const uint64_t got = dint_state_unlock_check_host(workload, &g, (const dint_lock_record *)(r.data() + 1), hd[0]);
    if (got != hd[1]) {
      printf("list %llu: refused at %llu, expected %llu\n", (unsigned long long)i, (unsigned long long)got, (unsigned long long)hd[1]);
      bad++;
    }
  }
  fclose(f);
  printf("%llu images, %llu lists, %d failures\n", (unsigned long long)n, (unsigned long long)lists, bad);
  return bad ? 1 : 0;
}
