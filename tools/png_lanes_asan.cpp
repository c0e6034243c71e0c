// The lane-parallel inflate's host twin under sanitizers: a stand-alone program, nothing of HIP and nothing loaded
// into Python.  It includes the core (csrc/png_decode_core.h) and the host entry points' source (csrc/png_decode_host.h) and
// runs, over the files named on the command line, the window rule (host_inflate_lanes: decode_subseq lane by lane and pass by
// pass, the commit token by token) at subsequences of 32 bits / 4 tokens, 64 / 8 and the compiled defaults, and holds bytes
// and status to the serial twin's (host_decode).  Every file, stream and result is a heap block of exactly its size, so that a
// read or a write one byte outside is reported.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iclimategan_amd/csrc \
//       tools/png_lanes_asan.cpp -o png_lanes_asan && ./png_lanes_asan FILE...
//
// tests/test_png_lanes_host.py::test_twin_under_sanitizers builds and runs it on every fourth case and on all broken ones.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "png_decode_host.h"

int main(int argc, char** argv) {
  using namespace png_dec;
  const int32_t settings[3][2] = {{32, 4}, {64, 8}, {(int32_t)SUBSEQ_BITS_DEFAULT, (int32_t)LANE_TOKENS_DEFAULT}};
  int decoded = 0, refused = 0, corrupt = 0;
  unsigned long windows = 0, passes = 0;
  for (int a = 1; a < argc; ++a) {
    FILE* fp = fopen(argv[a], "rb");
    if (!fp) return fprintf(stderr, "cannot open %s\n", argv[a]), 2;
    fseek(fp, 0, SEEK_END);
    const long size = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    uint8_t* file = static_cast<uint8_t*>(malloc(size > 0 ? (size_t)size : 1));
    if (size > 0 && fread(file, 1, (size_t)size, fp) != (size_t)size) return fprintf(stderr, "cannot read %s\n", argv[a]), 2;
    fclose(fp);
    cgan_png_desc d;
    int32_t status = -1;
    char why[200] = "";
    if (host_parse(file, (size_t)size, &d, &status, why, sizeof(why))) return fprintf(stderr, "%s: %s\n", argv[a], why), 2;
    if (status != CGAN_PNG_OK) {
      ++refused;
      free(file);
      continue;
    }
    uint8_t* stream = static_cast<uint8_t*>(malloc(d.stream_bytes));
    if (host_stream(file, (size_t)size, &d, stream, d.stream_bytes, why, sizeof(why))) return fprintf(stderr, "%s: %s\n", argv[a], why), 2;
    uint8_t* serial = static_cast<uint8_t*>(malloc(inflated_bytes(d)));
    uint8_t* pixels = static_cast<uint8_t*>(malloc(pixel_bytes(d)));
    if (host_decode(stream, &d, serial, pixels, &status, why, sizeof(why))) return fprintf(stderr, "%s: %s\n", argv[a], why), 2;
    for (const auto& set : settings) {
      uint8_t* inflated = static_cast<uint8_t*>(malloc(inflated_bytes(d)));
      uint32_t trailer = 0, stats[LANES_STATS];
      int32_t lanes_status = -1;
      if (host_inflate_lanes(stream, &d, set[0], set[1], inflated, &trailer, stats, &lanes_status, why, sizeof(why)))
        return fprintf(stderr, "%s: %s\n", argv[a], why), 2;
      if (lanes_status != status) return fprintf(stderr, "%s at %d / %d: status %d, the serial twin's is %d\n", argv[a], set[0], set[1], lanes_status, status), 1;
      if (status == CGAN_PNG_OK && memcmp(inflated, serial, inflated_bytes(d)) != 0)
        return fprintf(stderr, "%s at %d / %d: the bytes differ from the serial twin's\n", argv[a], set[0], set[1]), 1;
      if (stats[STAT_MAX_PASSES] > LANES) return fprintf(stderr, "%s: %u passes in one window\n", argv[a], stats[STAT_MAX_PASSES]), 1;
      windows += stats[STAT_WINDOWS], passes += stats[STAT_PASSES];
      free(inflated);
    }
    status == CGAN_PNG_OK ? ++decoded : ++corrupt;
    free(pixels), free(serial), free(stream), free(file);
  }
  printf("%d files: %d decoded, %d with a status from the decode, %d refused by the parser; %lu windows, %lu passes\n", argc - 1, decoded,
         corrupt, refused, windows, passes);
  return 0;
}
