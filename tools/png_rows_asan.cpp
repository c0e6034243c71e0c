// The PNG decoder's row path on the host under sanitizers: a stand-alone program, nothing of HIP and nothing
// loaded into Python.  It includes the core (csrc/png_decode_core.h) and the host entry points' source
// (csrc/png_decode_host.h) and runs them over the files named on the command line: parse, the IDAT payloads joined, the table
// of row offsets for a candidate, then the row twin (every row from its offset, bounded to its chunk; the serial decode where a
// row is refused; unfilter, Adler-32).  Every file, stream, table and result is a heap block of exactly its size, so that a
// read or a write one byte outside is reported.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iclimategan_amd/csrc \
//       tools/png_rows_asan.cpp -o png_rows_asan && ./png_rows_asan FILE...
//
// tests/test_png_rows_host.py::test_row_path_under_sanitizers builds and runs it on the framed, refused and broken files.
#include <stdio.h>
#include <stdlib.h>

#include "png_decode_host.h"

int main(int argc, char** argv) {
  int by_rows = 0, serial = 0, after_refusal = 0, corrupt = 0, refused = 0;
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
    int32_t status = -1, path = -1;
    char why[160] = "";
    if (png_dec::host_parse(file, (size_t)size, &d, &status, why, sizeof(why))) return fprintf(stderr, "%s: %s\n", argv[a], why), 2;
    if (status != CGAN_PNG_OK) {
      ++refused;
      free(file);
      continue;
    }
    uint8_t* stream = static_cast<uint8_t*>(malloc(d.stream_bytes));
    if (png_dec::host_stream(file, (size_t)size, &d, stream, d.stream_bytes, why, sizeof(why)))
      return fprintf(stderr, "%s: %s\n", argv[a], why), 2;
    uint32_t* table = nullptr;
    if (d.rows) {
      table = static_cast<uint32_t*>(malloc(sizeof(uint32_t) * (d.rows + 1)));
      if (png_dec::host_row_table(file, (size_t)size, &d, table, why, sizeof(why))) return fprintf(stderr, "%s: %s\n", argv[a], why), 2;
    }
    uint8_t* inflated = static_cast<uint8_t*>(malloc(png_dec::inflated_bytes(d)));
    uint8_t* pixels = static_cast<uint8_t*>(malloc(png_dec::pixel_bytes(d)));
    if (png_dec::host_decode_rows(stream, &d, table, inflated, pixels, &status, &path, why, sizeof(why)))
      return fprintf(stderr, "%s: %s\n", argv[a], why), 2;
    if (status != CGAN_PNG_OK) ++corrupt;
    path == 1 ? ++by_rows : (path == 2 ? ++after_refusal : ++serial);
    free(pixels), free(inflated), free(table), free(stream), free(file);
  }
  printf("%d files: %d by rows, %d serial, %d serial after a refusal, %d of them with a status from the decode, %d refused by the parser\n",
         argc - 1, by_rows, serial, after_refusal, corrupt, refused);
  return 0;
}
