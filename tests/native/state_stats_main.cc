// state_stats_main.cc -- the table report's host form (dint_state_stats_image_host: dint_amd/csrc/k_stats.hip over
// state_stats.h, behind dint_state_image_check_host of k_image.hip) as a stand-alone program for a sanitizer run.  It reads the
// file `python tests/test_state_stats_host.py FILE` writes -- the hand-built images of that test with the numpy form's reports --
// feeds every image to the host form and compares word for word; then the same image truncated and with a link bent, which
// must be refused.  No device call.  Build and run (host code only; nothing of it is loaded into python):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tests/native/state_stats_main.cc dint_amd/csrc/k_stats.hip dint_amd/csrc/k_image.hip -o state_stats_main
//   ./state_stats_main FILE
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
    const uint64_t bytes = hd[0], tables = hd[1], padded = (bytes + 7) / 8 * 8;
    std::vector<uint8_t> img(padded);  // (exactly the image's size would do: the host form is told `bytes`)
    std::vector<uint64_t> want(tables * 80);
    if (fread(img.data(), 1, padded, f) != padded || fread(want.data(), 8, want.size(), f) != want.size()) return 2;
    img.resize(bytes);
    img.shrink_to_fit();  // the sanitizer sees a read one byte past the image
    std::vector<dint_table_stats> out(tables);
    const int rc = dint_state_stats_image_host(img.data(), bytes, out.data(), (uint32_t)tables);
    if (rc != (int)tables || memcmp(out.data(), want.data(), want.size() * 8) != 0) {
      printf("image %llu: rc %d (%s), or a word differs\n", (unsigned long long)i, rc, g_err);
      bad++;
    }
    if (dint_state_stats_image_host(img.data(), bytes, out.data(), (uint32_t)tables - 1) != DINT_EINVAL) bad++;
    if (bytes > 400) {
      if (dint_state_stats_image_host(img.data(), bytes - 16, out.data(), (uint32_t)tables) != DINT_EINVAL) bad++;
      std::vector<uint8_t> bent(img);  // bytes 52..59 of every 64 behind the header overwritten: links, ids and values far outside
      for (uint64_t at = 320; at + 64 <= bytes; at += 64) memset(bent.data() + at + 52, 0xEE, 8);
      const int rb = dint_state_stats_image_host(bent.data(), bytes, out.data(), (uint32_t)tables);
      if (rb != DINT_EINVAL && rb != (int)tables) bad++;  // (refused by the check, or still an image: either way nothing outside it is read)
    }
  }
  fclose(f);
  printf("%llu images, %d failures\n", (unsigned long long)n, bad);
  return bad ? 1 : 0;
}
