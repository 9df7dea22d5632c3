// Untrusted-input hygiene of fdet_jpeg_scan_prepare (csrc/fdet_jpeg.hip): a stand-alone host program, meant to be built
// with the address and undefined-behaviour sanitizers.  No GPU is touched: prepare makes no HIP call.
//
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Iinclude \
//         pytorch-face-detection-from-scratch_amd/csrc/fdet_jpeg.hip tools/jpeg_prepare_check.cpp -o jpeg_prepare_check
//   ./jpeg_prepare_check [--prefixes] FILE...
//
// Every FILE is copied into a heap block of exactly its size (so that a read past bytes + n is a sanitizer report) and
// prepared into scan / segment buffers of exactly the documented capacities, then into capacities that are too small.
// --prefixes does the same for every prefix of every FILE.  The outcome codes are counted and printed; whatever a sound
// call may return is fine, the sanitizers judge the rest.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "fdet.h"

static std::map<int, long> g_outcomes;

static void one(const uint8_t* src, size_t n) {
  uint8_t* bytes = (uint8_t*)malloc(n ? n : 1);
  memcpy(bytes, src, n);
  fdet_jpeg_info_t info;
  const int irc = n ? fdet_jpeg_info(bytes, n, &info) : -1;
  long segs_needed = 1;
  if (irc == 0) {
    const long mcus = (long)info.mcus_x * info.mcus_y;
    const long ri = info.restart_interval ? info.restart_interval : mcus;
    segs_needed = (mcus + ri - 1) / ri;
  }
  const size_t full = ((n + 15) & ~(size_t)15) + 16 * (size_t)segs_needed;
  const size_t caps[4] = {full, full / 2, 16, 0};
  const long seg_caps[2] = {segs_needed, segs_needed > 1 ? segs_needed - 1 : 1};
  for (int ci = 0; ci < 4; ++ci) {
    for (int si = 0; si < 2; ++si) {
      const size_t cap = caps[ci];
      const long sc = seg_caps[si];
      uint8_t* scan = (uint8_t*)malloc(cap ? cap : 1);
      fdet_jpeg_huff_segment* segs = (fdet_jpeg_huff_segment*)malloc(sizeof(fdet_jpeg_huff_segment) * (size_t)sc);
      fdet_jpeg_huff_tables* tables = (fdet_jpeg_huff_tables*)malloc(sizeof(fdet_jpeg_huff_tables));
      size_t used = 0;
      int got = 0;
      const int rc = n ? fdet_jpeg_scan_prepare(bytes, n, scan, cap, &used, segs, (int)sc, &got, tables) : -1;
      if (ci == 0 && si == 0) {
        g_outcomes[rc] += 1;
        if (rc == 0) {                                   // what a caller relies on
          if (used > cap || used % 16 || got != segs_needed) { fprintf(stderr, "bad result sizes\n"); abort(); }
          size_t at = 0;
          for (int s = 0; s < got; ++s) {
            if ((size_t)segs[s].byte_offset != at || segs[s].byte_len < 0) { fprintf(stderr, "bad segment\n"); abort(); }
            at += ((size_t)segs[s].byte_len + 15) & ~(size_t)15;
          }
          if (at != used) { fprintf(stderr, "segments do not tile the scan\n"); abort(); }
        }
      }
      free(tables);
      free(segs);
      free(scan);
    }
  }
  free(bytes);
}

int main(int argc, char** argv) {
  bool prefixes = false;
  long files = 0, calls = 0;
  for (int a = 1; a < argc; ++a) {
    if (!strcmp(argv[a], "--prefixes")) { prefixes = true; continue; }
    FILE* f = fopen(argv[a], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
    std::vector<uint8_t> data;
    uint8_t buf[4096];
    size_t k;
    while ((k = fread(buf, 1, sizeof(buf), f)) > 0) data.insert(data.end(), buf, buf + k);
    fclose(f);
    ++files;
    if (prefixes) {
      for (size_t n = 0; n < data.size(); ++n, ++calls) one(data.data(), n);
    }
    one(data.data(), data.size());
    ++calls;
  }
  printf("%ld files, %ld inputs;", files, calls);
  for (auto& kv : g_outcomes) printf(" code %d: %ld", kv.first, kv.second);
  printf("\n");
  return 0;
}
