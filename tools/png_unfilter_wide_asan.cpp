// The wide unfilter's schedule on the host under sanitizers: a stand-alone program, nothing of HIP and nothing
// loaded into Python.  It includes the core (csrc/png_decode_core.h) and the host entry points' source
// (csrc/png_decode_host.h) and runs, for every file named on the command line: parse, the IDAT payloads joined, the serial twin
// (host_decode: inflate, unfilter, Adler-32), then host_unfilter_wide on the serial twin's inflated bytes and the stream's
// trailer with WAVES waves and a lag of LAG -- the schedule unfilter_kernel<WAVES, LAG> runs, every ring and `above` slot
// stamped with the chunk that wrote it.  The pixels and the status must be the serial twin's and no read may cross a barrier
// the wrong way.  Every file, stream and result is a heap block of exactly its size, so that a read or a write one byte outside
// is reported.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iclimategan_amd/csrc \
//       tools/png_unfilter_wide_asan.cpp -o png_unfilter_wide_asan && ./png_unfilter_wide_asan WAVES LAG FILE...
//
// tests/test_png_unfilter_wide_host.py::test_wide_schedule_under_sanitizers builds and runs it on that file's shape list.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "png_decode_host.h"

int main(int argc, char** argv) {
  if (argc < 3) return fprintf(stderr, "usage: %s WAVES LAG FILE...\n", argv[0]), 2;
  const int waves = atoi(argv[1]), lag = atoi(argv[2]);
  int intact = 0, corrupt = 0, not_inflated = 0;
  for (int a = 3; a < argc; ++a) {
    FILE* fp = fopen(argv[a], "rb");
    if (!fp) return fprintf(stderr, "cannot open %s\n", argv[a]), 2;
    fseek(fp, 0, SEEK_END);
    const long size = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    uint8_t* file = static_cast<uint8_t*>(malloc(size > 0 ? (size_t)size : 1));
    if (size > 0 && fread(file, 1, (size_t)size, fp) != (size_t)size) return fprintf(stderr, "cannot read %s\n", argv[a]), 2;
    fclose(fp);
    cgan_png_desc d;
    int32_t status = -1, wide_status = -1;
    char why[160] = "";
    if (png_dec::host_parse(file, (size_t)size, &d, &status, why, sizeof(why)) || status != CGAN_PNG_OK)
      return fprintf(stderr, "%s: %s\n", argv[a], why), 2;
    uint8_t* stream = static_cast<uint8_t*>(malloc(d.stream_bytes));
    if (png_dec::host_stream(file, (size_t)size, &d, stream, d.stream_bytes, why, sizeof(why)))
      return fprintf(stderr, "%s: %s\n", argv[a], why), 2;
    const size_t nin = png_dec::inflated_bytes(d), npx = png_dec::pixel_bytes(d);
    uint8_t* inflated = static_cast<uint8_t*>(malloc(nin));
    uint8_t* pixels = static_cast<uint8_t*>(malloc(npx));
    uint8_t* wide = static_cast<uint8_t*>(malloc(npx));
    memset(inflated, 0x55, nin), memset(pixels, 0x55, npx), memset(wide, 0xAA, npx);
    if (png_dec::host_decode(stream, &d, inflated, pixels, &status, why, sizeof(why))) return fprintf(stderr, "%s: %s\n", argv[a], why), 2;
    const bool inflate_failed = status != CGAN_PNG_OK && strcmp(why, "an invalid deflate stream") == 0;
    if (inflate_failed) {
      ++not_inflated;                                                   // the kernel is not run on such a file either
    } else {
      const uint32_t trailer = png_dec::be32(stream + d.stream_bytes - 4);
      const int rc = png_dec::host_unfilter_wide(d, inflated, trailer, waves, lag, wide, &wide_status, why, sizeof(why));
      if (rc) return fprintf(stderr, "%s: waves %d, lag %d: %s\n", argv[a], waves, lag, why), rc == -2 ? 3 : 2;
      if (wide_status != status) return fprintf(stderr, "%s: status %d, the serial twin's is %d\n", argv[a], wide_status, status), 4;
      if (status == CGAN_PNG_OK && memcmp(wide, pixels, npx) != 0) return fprintf(stderr, "%s: the pixels differ\n", argv[a]), 4;
      status == CGAN_PNG_OK ? ++intact : ++corrupt;
    }
    free(wide), free(pixels), free(inflated), free(stream), free(file);
  }
  printf("waves %d, lag %d: %d files: %d equal to the serial twin, %d corrupt in both, %d not inflated\n", waves, lag, argc - 3, intact, corrupt,
         not_inflated);
  return 0;
}
