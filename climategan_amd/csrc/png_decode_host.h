// The host entry points of the PNG decoder without anything of HIP: png_decode.hip wraps them into the C ABI
// (cgan_png_parse_host, cgan_png_stream_host, cgan_png_decode_host, and for row-framed files, DESIGN 4.22,
// cgan_png_row_table_host and cgan_png_decode_rows_host), tools/png_decode_asan.cpp and tools/png_rows_asan.cpp run the same
// text under sanitizers.  Each returns 0 or -1 (an argument refused, the reason in `why`); the file's status goes to *status.
#pragma once
#include "png_decode_core.h"

namespace png_dec {

inline int host_parse(const uint8_t* file, size_t file_bytes, cgan_png_desc* desc, int32_t* status, char* why, size_t why_len) {
  if (!file || !desc || !status) return snprintf(why, why_len, "null pointer"), -1;
  *status = walk(file, file_bytes, desc, nullptr, 0, why, why_len);
  return 0;
}

inline int host_stream(const uint8_t* file, size_t file_bytes, const cgan_png_desc* desc, uint8_t* dst, size_t dst_bytes, char* why,
                       size_t why_len) {
  if (!file || !desc || !dst) return snprintf(why, why_len, "null pointer"), -1;
  if (dst_bytes < desc->stream_bytes) return snprintf(why, why_len, "dst holds %zu bytes, %u are needed", dst_bytes, desc->stream_bytes), -1;
  cgan_png_desc again;
  if (walk(file, file_bytes, &again, dst, desc->stream_bytes, why, why_len) != CGAN_PNG_OK || again.stream_bytes != desc->stream_bytes)
    return snprintf(why, why_len, "the descriptor is not this file's"), -1;
  return 0;
}

// a candidate's table of rows + 1 stream offsets (walk): the descriptor must be this file's
inline int host_row_table(const uint8_t* file, size_t file_bytes, const cgan_png_desc* desc, uint32_t* table, char* why, size_t why_len) {
  if (!file || !desc || !table) return snprintf(why, why_len, "null pointer"), -1;
  if (!desc_ok(*desc) || desc->rows == 0) return snprintf(why, why_len, "not the descriptor of a row-framed candidate"), -1;
  cgan_png_desc again;
  if (walk(file, file_bytes, &again, nullptr, 0, why, why_len, table, desc->rows + 1) != CGAN_PNG_OK ||
      again.stream_bytes != desc->stream_bytes || again.rows != desc->rows || again.height != desc->height)
    return snprintf(why, why_len, "the descriptor is not this file's"), -1;
  return 0;
}

// the tokens of one stream, row or tail executed serially: out[0] is the first byte this run of the reader produces
inline void host_run(Inflate& s, Tables& t, const uint8_t* stream, uint8_t* out) {
  uint32_t at = 0;
  Token tok[64];
  while (s.phase != PHASE_DONE && !s.err) {
    const uint32_t nt = decode_tokens(s, t, tok, 64);
    for (uint32_t i = 0; i < nt; ++i) {
      const Token k = tok[i];
      for (uint32_t j = 0; j < k.len; ++j, ++at)          // at + len <= the limit, arg <= at: decode_tokens checked it
        out[at] = k.kind == TOK_LITERAL ? k.lit : (k.kind == TOK_MATCH ? out[at - k.arg] : stream[k.arg + j]);
    }
  }
}

// the second stage: the inflated rows -> the pixels, and the Adler-32 of the bytes read against the stream's trailer
inline int host_unfilter(const cgan_png_desc& d, const uint8_t* inflated, uint32_t trailer, uint8_t* pixels, int32_t* status, char* why,
                         size_t why_len) {
  const uint32_t total = inflated_bytes(d), rb = row_bytes(d), bpp = bytes_per_pixel(d);
  Adler ad;
  ad.start();
  bool bad_filter = false;
  for (uint32_t y = 0; y < (uint32_t)d.height; ++y) {
    const uint8_t* row = inflated + (size_t)y * (1 + rb);
    const uint32_t filter = row[0];
    if (filter > 4) bad_filter = true;
    ad.byte(filter);
    uint32_t a = 0, c = 0;
    for (uint32_t x = 0; x < (uint32_t)d.width; ++x) {
      uint32_t raw = 0, b = 0;
      for (uint32_t k = 0; k < bpp; ++k) {
        raw |= (uint32_t)row[1 + x * bpp + k] << (8 * k);
        ad.byte(row[1 + x * bpp + k]);
      }
      uint8_t* px = pixels + ((size_t)y * d.width + x) * bpp;
      if (y > 0)
        for (uint32_t k = 0; k < bpp; ++k) b |= (uint32_t)(px - rb)[d.bit_depth == 16 ? 1 - k : k] << (8 * k);
      const uint32_t v = unfilter_pixel(filter, raw, a, b, c);
      for (uint32_t k = 0; k < bpp; ++k) px[d.bit_depth == 16 ? 1 - k : k] = (uint8_t)(v >> (8 * k));      // 16 bits: host order
      a = v, c = b;
    }
    ad.end_piece(total - (y + 1) * (1 + rb));
  }
  if (adler_value(ad.s1, ad.s2, total) != trailer) {
    *status = CGAN_PNG_CORRUPT;
    return snprintf(why, why_len, "Adler-32 mismatch"), 0;
  }
  if (bad_filter) {
    *status = CGAN_PNG_CORRUPT;
    return snprintf(why, why_len, "a filter byte above 4"), 0;
  }
  return 0;
}

// The twin: the kernels' two stages one after the other, every token and every pixel taken serially.
//   inflated: inflated_bytes(desc) bytes, pixels: pixel_bytes(desc) bytes
inline int host_decode(const uint8_t* stream, const cgan_png_desc* desc, uint8_t* inflated, uint8_t* pixels, int32_t* status, char* why,
                       size_t why_len) {
  if (!stream || !desc || !inflated || !pixels || !status) return snprintf(why, why_len, "null pointer"), -1;
  if (!desc_ok(*desc)) return snprintf(why, why_len, "not a descriptor the parser produces"), -1;
  const cgan_png_desc& d = *desc;
  *status = CGAN_PNG_OK;
  why[0] = 0;
  Inflate s;
  Tables* t = new Tables;
  s.start(stream, d.stream_bytes, inflated_bytes(d));
  host_run(s, *t, stream, inflated);
  delete t;
  if (s.err) {
    *status = CGAN_PNG_CORRUPT;
    return snprintf(why, why_len, "an invalid deflate stream"), 0;
  }
  return host_unfilter(d, inflated, s.adler, pixels, status, why, why_len);
}

// Row-framed files: the row kernel's work row by row -- every row and the tail from its table offset, bounded
// to its chunk, under the row-end rule -- and, where any of them is refused, the serial decode above, whose verdict stands.
//   table: rows + 1 offsets for a candidate (cgan_png_row_table_host), not read otherwise.  *path: 0 serial, 1 rows, 2 serial
//   after the row path refused.
inline int host_decode_rows(const uint8_t* stream, const cgan_png_desc* desc, const uint32_t* table, uint8_t* inflated, uint8_t* pixels,
                            int32_t* status, int32_t* path, char* why, size_t why_len) {
  if (!stream || !desc || !inflated || !pixels || !status || !path) return snprintf(why, why_len, "null pointer"), -1;
  if (!desc_ok(*desc)) return snprintf(why, why_len, "not a descriptor the parser produces"), -1;
  const cgan_png_desc& d = *desc;
  *path = 0;
  if (d.rows == 0) return host_decode(stream, desc, inflated, pixels, status, why, why_len);
  if (!table || !table_ok(d, table)) return snprintf(why, why_len, "not this descriptor's row table"), -1;
  const uint32_t rb = row_bytes(d);
  Tables* t = new Tables;
  Inflate s;
  bool refused = false;
  for (uint32_t k = 0; k <= d.rows && !refused; ++k) {
    const bool tail = k == d.rows;
    s.start_row(stream, table[k], tail ? d.stream_bytes : table[k + 1], tail ? 0u : 1u + rb, tail ? MODE_TAIL : MODE_ROW);
    host_run(s, *t, stream, inflated + (size_t)(tail ? 0 : k) * (1 + rb));
    refused = s.err != 0;
  }
  delete t;
  if (refused) {
    *path = 2;
    return host_decode(stream, desc, inflated, pixels, status, why, why_len);
  }
  *path = 1;
  *status = CGAN_PNG_OK;
  why[0] = 0;
  return host_unfilter(d, inflated, s.adler, pixels, status, why, why_len);
}

}  // namespace png_dec
