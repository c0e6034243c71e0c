// Tables and serial logic of the JPEG encoder (jpeg.hip): plain functions on plain arrays, the same text for
// the host (cgan_jpeg_tables, cgan_jpeg_scan_host: tested without a GPU) and for the kernels.
//
//   quantisation     base_quant (ITU-T T.81 Annex K.1 / K.2, natural order), quality_scale + scaled_quant (libjpeg's rule)
//   order            zigzag (scan position -> natural index)
//   entropy code     huff_bits / huff_vals (Annex K.3), build_codes (-> (length << 16) | code per symbol),
//                    code_block (the codes of one block, given its 64 coefficients and the previous DC, into a sink)
//   container        geometry, header_bytes, write_headers (SOI .. SOS), bound arithmetic
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JPEG_HD __host__ __device__
#else
#define JPEG_HD
#endif

namespace jpeg_tab {

constexpr int DC_LUMA = 0, AC_LUMA = 1, DC_CHROMA = 2, AC_CHROMA = 3;     // the four code tables, in the order of the DHTs
// the most bits one block can take: DC 11 + 11, every AC 16 + 10 (the longest code and the widest value)
constexpr uint32_t BLOCK_MAX_BITS = 22u + 63u * 26u;

// Annex K.1 (table 0, luminance) and K.2 (table 1, chrominance), natural (row-major) order
JPEG_HD inline int base_quant(int table, int i) {
  constexpr uint8_t t[2][64] = {
      {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
       14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
       49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
      {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
       47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
       99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
  return t[table][i];
}

// natural index of scan position k
JPEG_HD inline int zigzag(int k) {
  constexpr uint8_t t[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return t[k];
}

// libjpeg's jpeg_quality_scaling and jpeg_add_quant_table (baseline: 1 .. 255)
JPEG_HD inline int quality_scale(int quality) { return quality < 50 ? 5000 / quality : 200 - 2 * quality; }
JPEG_HD inline int scaled_quant(int table, int i, int quality) {
  const int v = (base_quant(table, i) * quality_scale(quality) + 50) / 100;
  return v < 1 ? 1 : (v > 255 ? 255 : v);
}

// Annex K.3: how many codes of each length 1 .. 16, then the symbols in code order
JPEG_HD inline int huff_bits(int table, int len_minus_1) {
  constexpr uint8_t t[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
                                {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
  return t[table][len_minus_1];
}
JPEG_HD inline int huff_count(int table) { return (table & 1) ? 162 : 12; }
JPEG_HD inline int huff_val(int table, int k) {
  constexpr uint8_t ac_luma[162] = {
      0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
      0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
      0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
      0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
      0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
      0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
      0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
      0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
      0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
  constexpr uint8_t ac_chroma[162] = {
      0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
      0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
      0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
      0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
      0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
      0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
      0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
      0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
      0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
  if (!(table & 1)) return k;              // both DC tables: the categories 0 .. 11 in order
  return table == AC_LUMA ? ac_luma[k] : ac_chroma[k];
}

// A code table expanded: out[symbol] = (length << 16) | code, 0 for a symbol without a code (Annex C: codes of one length
// are consecutive, and the first of a length is twice the one after the last of the length before)
JPEG_HD inline void build_codes(int table, uint32_t* out /* [256] */) {
  for (int s = 0; s < 256; ++s) out[s] = 0;
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < huff_bits(table, len - 1); ++i, ++k, ++code) out[huff_val(table, k)] = ((uint32_t)len << 16) | code;
    code <<= 1;
  }
}

// the category of a value: the bits of its magnitude (0 for 0)
JPEG_HD inline int category(int v) {
  uint32_t a = (uint32_t)(v < 0 ? -v : v);
  int s = 0;
  while (a) ++s, a >>= 1;
  return s;
}

// The codes of one block into sink(value, bits) (value's low `bits` bits enter the stream most significant first): the
// DC difference against prev_dc, then the AC values in zig-zag order as (run, category) symbols with ZRL for runs of 16
// zeros and EOB behind the last non-zero value.  coef: 64 values, natural order.
template <typename Sink>
JPEG_HD inline void code_block(const int16_t* coef, int prev_dc, const uint32_t* dc_codes, const uint32_t* ac_codes,
                               Sink& sink) {
  {
    const int diff = (int)coef[0] - prev_dc;
    const int s = category(diff);
    const uint32_t extra = (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1u);
    const uint32_t e = dc_codes[s];
    sink(((e & 0xffffu) << s) | extra, (e >> 16) + (uint32_t)s);
  }
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = coef[zigzag(k)];
    if (v == 0) {
      ++run;
      continue;
    }
    for (; run >= 16; run -= 16) sink(ac_codes[0xF0] & 0xffffu, ac_codes[0xF0] >> 16);
    const int s = category(v);
    const uint32_t extra = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u);
    const uint32_t e = ac_codes[(run << 4) | s];
    sink(((e & 0xffffu) << s) | extra, (e >> 16) + (uint32_t)s);
    run = 0;
  }
  if (run > 0) sink(ac_codes[0] & 0xffffu, ac_codes[0] >> 16);
}
struct BitCounter {
  uint32_t bits = 0;
  JPEG_HD void operator()(uint32_t, uint32_t n) { bits += n; }
};
JPEG_HD inline uint32_t block_bits(const int16_t* coef, int prev_dc, const uint32_t* dc_codes, const uint32_t* ac_codes) {
  BitCounter c;
  code_block(coef, prev_dc, dc_codes, ac_codes, c);
  return c.bits;
}

// ---- the frame ---------------------------------------------------------------------------------------------------------
// An MCU is 8 x 8 pixels (grey, 4:4:4) or 16 x 16 (4:2:0); its blocks in scan order are ny luma blocks (raster order within
// the MCU) and then one block of each chroma component.  The coefficient layout of cgan_jpeg_coefficients_u8 /
// cgan_jpeg_scan_host: the components one after the other, each its blocks in raster order over the MCU-padded frame
// (luma: mcus_y * v rows of mcus_x * v blocks, v = 2 for 4:2:0; chroma: mcus_y rows of mcus_x), 64 values per block.
struct Geometry {
  int ncomp, v, mcu, mcus_x, mcus_y, ny, bpm;        // bpm: blocks per MCU
  int64_t luma_blocks, chroma_blocks, blocks;        // per image
};
JPEG_HD inline Geometry geometry(int h, int w, int c, int sub420) {
  Geometry g;
  g.ncomp = c;
  g.v = (c == 3 && sub420) ? 2 : 1;
  g.mcu = 8 * g.v;
  g.mcus_x = (w + g.mcu - 1) / g.mcu;
  g.mcus_y = (h + g.mcu - 1) / g.mcu;
  g.ny = g.v * g.v;
  g.bpm = g.ny + (c == 3 ? 2 : 0);
  g.luma_blocks = (int64_t)g.mcus_x * g.mcus_y * g.ny;
  g.chroma_blocks = c == 3 ? (int64_t)g.mcus_x * g.mcus_y : 0;
  g.blocks = g.luma_blocks + 2 * g.chroma_blocks;
  return g;
}
// block k (scan order) of the MCU (my, mx) -> its index in the coefficient layout, and its component
JPEG_HD inline int64_t coef_block(const Geometry& g, int my, int mx, int k, int& comp) {
  if (k < g.ny) {
    comp = 0;
    return ((int64_t)my * g.v + k / g.v) * ((int64_t)g.mcus_x * g.v) + (int64_t)mx * g.v + k % g.v;
  }
  comp = k - g.ny + 1;
  return g.luma_blocks + (int64_t)(comp - 1) * g.chroma_blocks + (int64_t)my * g.mcus_x + mx;
}

// SOI, APP0, DQT per table, SOF0, DHT per table, DRI, SOS -- the segments in libjpeg's order
JPEG_HD inline uint32_t header_bytes(int c) { return c == 3 ? 2u + 18u + 2u * 69u + 19u + 2u * 216u + 6u + 14u : 2u + 18u + 69u + 13u + 216u + 6u + 10u; }
// the most bytes the entropy-coded data of one MCU row can have: BLOCK_MAX_BITS per block, padded to a byte, every byte an
// FF that is stuffed
JPEG_HD inline uint32_t row_max_bytes(const Geometry& g) {
  return 2u * (uint32_t)(((uint64_t)g.mcus_x * g.bpm * BLOCK_MAX_BITS + 7u) / 8u);
}
// one file: headers, every MCU row's data, an RSTm between rows, EOI
JPEG_HD inline uint64_t file_max_bytes(const Geometry& g) {
  return header_bytes(g.ncomp) + (uint64_t)g.mcus_y * row_max_bytes(g) + 2u * (uint64_t)(g.mcus_y - 1) + 2u;
}

JPEG_HD inline uint8_t* put_marker(uint8_t* p, int marker, int length) {
  p[0] = 0xFF, p[1] = (uint8_t)marker, p[2] = (uint8_t)(length >> 8), p[3] = (uint8_t)length;
  return p + 4;
}
// SOI .. SOS at p (header_bytes(c) bytes); returns the byte behind them
JPEG_HD inline uint8_t* write_headers(uint8_t* p, int h, int w, int c, int sub420, int quality) {
  const Geometry g = geometry(h, w, c, sub420);
  p[0] = 0xFF, p[1] = 0xD8;
  p = put_marker(p + 2, 0xE0, 16);
  const uint8_t jfif[12] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1};      // version 1.01, no unit, density 1 : 1
  for (int i = 0; i < 12; ++i) p[i] = jfif[i];
  p[12] = 0, p[13] = 0;                                                      // no thumbnail
  p += 14;
  for (int t = 0; t < (c == 3 ? 2 : 1); ++t) {
    p = put_marker(p, 0xDB, 67);
    *p++ = (uint8_t)t;                                                       // 8-bit entries, table t
    for (int k = 0; k < 64; ++k) *p++ = (uint8_t)scaled_quant(t, zigzag(k), quality);
  }
  p = put_marker(p, 0xC0, 8 + 3 * c);
  p[0] = 8, p[1] = (uint8_t)(h >> 8), p[2] = (uint8_t)h, p[3] = (uint8_t)(w >> 8), p[4] = (uint8_t)w, p[5] = (uint8_t)c;
  p += 6;
  for (int i = 0; i < c; ++i) {
    p[0] = (uint8_t)(i + 1);
    p[1] = (uint8_t)(i == 0 ? (g.v << 4) | g.v : 0x11);
    p[2] = (uint8_t)(i == 0 ? 0 : 1);
    p += 3;
  }
  for (int t = 0; t < (c == 3 ? 4 : 2); ++t) {
    const int n = huff_count(t);
    p = put_marker(p, 0xC4, 19 + n);
    *p++ = (uint8_t)(((t & 1) << 4) | (t >> 1));                             // class (0 DC, 1 AC), identifier
    for (int i = 0; i < 16; ++i) *p++ = (uint8_t)huff_bits(t, i);
    for (int i = 0; i < n; ++i) *p++ = (uint8_t)huff_val(t, i);
  }
  p = put_marker(p, 0xDD, 4);
  p[0] = (uint8_t)(g.mcus_x >> 8), p[1] = (uint8_t)g.mcus_x;
  p = put_marker(p + 2, 0xDA, 6 + 2 * c);
  *p++ = (uint8_t)c;
  for (int i = 0; i < c; ++i) {
    *p++ = (uint8_t)(i + 1);
    *p++ = (uint8_t)(i == 0 ? 0x00 : 0x11);
  }
  p[0] = 0, p[1] = 63, p[2] = 0;                                             // the whole spectrum, no approximation
  return p + 3;
}

// ---- the whole file on the host, from coefficients in the layout above --------------------------------------------------
struct ByteSink {                     // most significant bit first, FF -> FF 00
  uint8_t* out;
  uint64_t cap, n = 0;
  uint32_t acc = 0, nacc = 0;
  JPEG_HD void byte(uint32_t b) {
    if (n < cap) out[n] = (uint8_t)b;
    ++n;
  }
  JPEG_HD void operator()(uint32_t v, uint32_t bits) {
    for (uint32_t i = bits; i-- > 0;) {
      acc = (acc << 1) | ((v >> i) & 1u);
      if (++nacc == 8) {
        byte(acc);
        if (acc == 0xFFu) byte(0);
        acc = 0, nacc = 0;
      }
    }
  }
  JPEG_HD void pad_ones() {
    if (nacc) (*this)((1u << (8u - nacc)) - 1u, 8u - nacc);
  }
};
// returns the file's length; bytes past cap are counted and not written
inline uint64_t scan_host(const int16_t* coef, int h, int w, int c, int sub420, int quality, uint8_t* out, uint64_t cap) {
  const Geometry g = geometry(h, w, c, sub420);
  uint8_t head[640];
  const uint64_t hb = (uint64_t)(write_headers(head, h, w, c, sub420, quality) - head);
  ByteSink sink{out, cap};
  for (uint64_t i = 0; i < hb; ++i) sink.byte(head[i]);
  uint32_t codes[4][256];
  for (int t = 0; t < 4; ++t) build_codes(t, codes[t]);
  for (int my = 0; my < g.mcus_y; ++my) {
    int dc[3] = {0, 0, 0};
    for (int mx = 0; mx < g.mcus_x; ++mx)
      for (int k = 0; k < g.bpm; ++k) {
        int comp;
        const int16_t* b = coef + 64 * coef_block(g, my, mx, k, comp);
        code_block(b, dc[comp], codes[comp ? DC_CHROMA : DC_LUMA], codes[comp ? AC_CHROMA : AC_LUMA], sink);
        dc[comp] = b[0];
      }
    sink.pad_ones();
    if (my + 1 < g.mcus_y) sink.byte(0xFF), sink.byte(0xD0 + (my & 7));
  }
  sink.byte(0xFF), sink.byte(0xD9);
  return sink.n;
}

}  // namespace jpeg_tab
