// The JPEG decoder's host side under sanitizers: a stand-alone program, nothing of HIP and nothing loaded into
// Python.  It includes the core (csrc/jpeg_decode_core.h) and the host entry points' source (csrc/jpeg_decode_host.h) and runs
// them over the files named on the command line: parse, then the coefficient decode at 4, 16 and the default bytes per
// subsequence, uncapped and with a round cap of 1, and the integer reconstruction of what decoded.  Every file is copied into
// a heap block of exactly its size and the coefficients into one of exactly theirs, so that a read or a write one byte
// outside is reported.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iclimategan_amd/csrc \
//       tools/jpeg_decode_asan.cpp -o jpeg_decode_asan && ./jpeg_decode_asan FILE...
//
// tests/test_jpeg_decode_host.py::test_core_under_sanitizers builds and runs it on the corpus and on the cut / changed files.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "jpeg_decode_host.h"

int main(int argc, char** argv) {
  int decoded = 0, refused = 0, corrupt = 0;
  for (int a = 1; a < argc; ++a) {
    FILE* fp = fopen(argv[a], "rb");
    if (!fp) return fprintf(stderr, "cannot open %s\n", argv[a]), 2;
    fseek(fp, 0, SEEK_END);
    const long size = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    uint8_t* file = static_cast<uint8_t*>(malloc(size > 0 ? (size_t)size : 1));
    if (size > 0 && fread(file, 1, (size_t)size, fp) != (size_t)size) return fprintf(stderr, "cannot read %s\n", argv[a]), 2;
    fclose(fp);
    cgan_jpeg_desc d;
    int32_t status = -1;
    char why[160] = "";
    if (jpeg_dec::host_parse(file, (size_t)size, &d, &status, why, sizeof(why))) return fprintf(stderr, "%s: %s\n", argv[a], why), 2;
    if (status != CGAN_JPEG_OK) {
      ++refused;
      free(file);
      continue;
    }
    const jpeg_dec::Frame f = jpeg_dec::frame(d);
    const size_t count = 64 * (size_t)f.blocks;
    bool ok = false;
    for (int subseq : {4, 16, 0})
      for (int cap : {0, 1}) {
        int16_t* coef = static_cast<int16_t*>(malloc(sizeof(int16_t) * count));
        int32_t rounds = 0;
        if (jpeg_dec::host_decode_coefficients(file, (size_t)size, &d, subseq, cap, coef, count, &rounds, &status, why, sizeof(why)))
          return fprintf(stderr, "%s: %s\n", argv[a], why), 2;
        if (status == CGAN_JPEG_OK && subseq == 0 && cap == 0) {
          ok = true;
          std::vector<uint8_t> px(64);
          for (int64_t b = 0; b < f.blocks; ++b) {
            const int comp = (f.ncomp == 3 && b >= f.off[1]) ? (b >= f.off[2] ? 2 : 1) : 0;
            jpeg_dec::idct_block(coef + 64 * b, d.quant[comp], px.data());
          }
        }
        free(coef);
      }
    ok ? ++decoded : ++corrupt;
    free(file);
  }
  printf("%d files: %d decoded, %d with a status from the decode, %d refused by the parser\n", argc - 1, decoded, corrupt, refused);
  return 0;
}
