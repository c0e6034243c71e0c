// The host entry points of the PNG decoder without anything of HIP: png_decode.hip wraps them into the C ABI
// (cgan_png_parse_host, cgan_png_stream_host, cgan_png_decode_host), tools/png_decode_asan.cpp runs the same text under
// sanitizers.  Each returns 0 or -1 (an argument refused, the reason in `why`); the file's status goes to *status.
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

// The twin: the kernels' two stages one after the other, every token and every pixel taken serially.
//   inflated: inflated_bytes(desc) bytes, pixels: pixel_bytes(desc) bytes
inline int host_decode(const uint8_t* stream, const cgan_png_desc* desc, uint8_t* inflated, uint8_t* pixels, int32_t* status, char* why,
                       size_t why_len) {
  if (!stream || !desc || !inflated || !pixels || !status) return snprintf(why, why_len, "null pointer"), -1;
  if (!desc_ok(*desc)) return snprintf(why, why_len, "not a descriptor the parser produces"), -1;
  const cgan_png_desc& d = *desc;
  const uint32_t total = inflated_bytes(d), rb = row_bytes(d), bpp = bytes_per_pixel(d);
  *status = CGAN_PNG_OK;
  why[0] = 0;
  Inflate s;
  Tables* t = new Tables;
  s.start(stream, d.stream_bytes, total);
  uint32_t at = 0;
  Token tok[64];
  while (s.phase != PHASE_DONE && !s.err) {
    const uint32_t nt = decode_tokens(s, *t, tok, 64);
    for (uint32_t i = 0; i < nt; ++i) {
      const Token k = tok[i];
      for (uint32_t j = 0; j < k.len; ++j, ++at)          // at + len <= total: decode_tokens checked it
        inflated[at] = k.kind == TOK_LITERAL ? k.lit : (k.kind == TOK_MATCH ? inflated[at - k.arg] : stream[k.arg + j]);
    }
  }
  delete t;
  if (s.err) {
    *status = CGAN_PNG_CORRUPT;
    return snprintf(why, why_len, "an invalid deflate stream"), 0;
  }
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
  if (adler_value(ad.s1, ad.s2, total) != s.adler) {
    *status = CGAN_PNG_CORRUPT;
    return snprintf(why, why_len, "Adler-32 mismatch"), 0;
  }
  if (bad_filter) {
    *status = CGAN_PNG_CORRUPT;
    return snprintf(why, why_len, "a filter byte above 4"), 0;
  }
  return 0;
}

}  // namespace png_dec
