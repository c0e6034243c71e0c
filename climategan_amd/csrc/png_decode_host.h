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

// The token executor: k's bytes to out[at ..] -> the byte behind them.  out[0] is the first byte of the extent (the stream's,
// the row's); whoever hands the token over has checked at + len <= the extent's bytes and arg <= at (decode_tokens,
// token_refused) and a stored run against the stream's end (block_header).
inline uint32_t host_execute(const Token& k, const uint8_t* stream, uint8_t* out, uint32_t at) {
  for (uint32_t j = 0; j < k.len; ++j, ++at)
    out[at] = k.kind == TOK_LITERAL ? k.lit : (k.kind == TOK_MATCH ? out[at - k.arg] : stream[k.arg + j]);
  return at;
}

// the tokens of one stream, row or tail executed serially: out[0] is the first byte this run of the reader produces
inline void host_run(Inflate& s, Tables& t, const uint8_t* stream, uint8_t* out) {
  uint32_t at = 0;
  Token tok[64];
  while (s.phase != PHASE_DONE && !s.err) {
    const uint32_t nt = decode_tokens(s, t, tok, 64);
    for (uint32_t i = 0; i < nt; ++i) at = host_execute(tok[i], stream, out, at);
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

// The wide unfilter kernel's schedule run on the host: pass by pass, chunk by chunk, wave by wave, step by step,
// lane by lane, with the core's unf_* functions for every index, as unfilter_kernel<waves, lag> does.  What a barrier orders
// on the device is checked here: every ring and `above` slot carries the pixel it holds and the chunk that wrote it, and a
// read that finds another pixel (never written, or written again already) or a write of the same chunk (no barrier between
// the waves) is a violation: -2, the reason in `why`.  -1: an argument refused.  The status as host_unfilter sets it.
inline int host_unfilter_wide(const cgan_png_desc& d, const uint8_t* inflated, uint32_t trailer, int waves, int lag, uint8_t* pixels,
                              int32_t* status, char* why, size_t why_len) {
  if (!inflated || !pixels || !status) return snprintf(why, why_len, "null pointer"), -1;
  if (!desc_ok(d)) return snprintf(why, why_len, "not a descriptor the parser produces"), -1;
  if (!unf_params_ok(waves, lag))
    return snprintf(why, why_len, "waves = %d, lag = %d: 1 .. %d waves and a lag that is a multiple of %d, %d .. %d, expected", waves, lag,
                    UNF_MAX_WAVES, UNF_PREFETCH, UNF_PREFETCH, 8 * UNF_PREFETCH), -1;
  struct Slot {
    uint32_t v;
    int64_t pixel, chunk;      // which pixel of which pass (pass * MAX_DIM + x), written in which chunk (counted over the passes)
  };
  struct Lane {
    uint32_t cur, prev, above_left, filter;
    Adler ad;
    bool bad;
  };
  const int W = d.width, H = d.height, L = UNF_LANES;
  const uint32_t bpp = bytes_per_pixel(d), rb = row_bytes(d), total = inflated_bytes(d), ring_words = unf_ring_words(lag);
  const bool swap = d.bit_depth == 16;
  const uint32_t passes = unf_passes(H, waves), chunks = unf_chunks(W, waves, lag);
  Slot* above = new Slot[CGAN_PNG_MAX_DIM];
  Slot* ring = new Slot[(size_t)waves * ring_words];
  Lane* lanes = new Lane[(size_t)waves * L];
  uint32_t* shifted = new uint32_t[2 * L];                 // what __shfl_up hands every lane: the values of the step before
  for (int i = 0; i < CGAN_PNG_MAX_DIM; ++i) above[i] = Slot{0, -1, -1};
  for (size_t i = 0; i < (size_t)waves * ring_words; ++i) ring[i] = Slot{0, -1, -1};
  for (int i = 0; i < waves * L; ++i) {
    lanes[i].ad.start();
    lanes[i].bad = false;
  }
  int rc = 0;
  auto read_slot = [&](const Slot& s, int64_t pixel, int64_t chunk, const char* what, int wave, int x) -> uint32_t {
    if (rc == 0 && s.pixel != pixel)
      rc = (snprintf(why, why_len, "wave %d reads pixel %d of %s, which %s", wave, x, what, s.pixel < 0 ? "was never written" : "holds another pixel"), -2);
    else if (rc == 0 && s.chunk >= chunk)
      rc = (snprintf(why, why_len, "wave %d reads pixel %d of %s in the chunk that wrote it", wave, x, what), -2);
    return s.v;
  };
  for (uint32_t p = 0; p < passes && rc == 0; ++p) {
    for (int j = 0; j < waves; ++j)
      for (int r = 0; r < L; ++r) {
        Lane& l = lanes[j * L + r];
        const int y = unf_row(p, j, r, waves);
        l.filter = y < H ? inflated[(size_t)y * (1 + rb)] : 0u;
        if (y < H) l.ad.byte(l.filter);
        l.bad = l.bad || l.filter > 4;
        l.cur = l.prev = l.above_left = 0;
      }
    for (uint32_t c = 0; c < chunks && rc == 0; ++c) {
      const int64_t chunk = (int64_t)p * chunks + c;
      for (int j = 0; j < waves; ++j) {
        const int t0 = (int)(c * UNF_PREFETCH) - unf_wave_offset(j, lag);
        if (unf_wave_idle(unf_row(p, j, 0, waves), H, t0, W)) continue;
        for (int u = 0; u < UNF_PREFETCH; ++u) {
          for (int r = 0; r < L; ++r) shifted[r] = lanes[j * L + r].cur, shifted[L + r] = lanes[j * L + r].prev;
          for (int r = 0; r < L; ++r) {
            Lane& l = lanes[j * L + r];
            const int y = unf_row(p, j, r, waves), x = t0 + u - r;
            const bool live = y < H, active = live && x >= 0 && x < W;
            uint32_t b = r ? shifted[r - 1] : 0u, cc = r ? shifted[L + r - 1] : 0u;
            if (r == 0) {
              cc = l.above_left;
              b = 0u;
              if (active) {
                const int64_t pixel = (int64_t)p * CGAN_PNG_MAX_DIM + x;
                if (j > 0) {
                  b = read_slot(ring[(size_t)j * ring_words + unf_ring_index(x, ring_words)], pixel, chunk, "its ring", j, x);
                } else if (p > 0) {
                  b = read_slot(above[unf_above_index(x)], pixel - CGAN_PNG_MAX_DIM, chunk, "the row above the pass", j, x);
                }
              }
              l.above_left = b;
            }
            uint32_t v = 0;
            if (active) {
              const uint8_t* row = inflated + (size_t)y * (1 + rb);          // inside the inflated extent: y < H, x < W
              uint32_t raw = 0;
              for (uint32_t k = 0; k < bpp; ++k) raw |= (uint32_t)row[1 + (uint32_t)x * bpp + k] << (8 * k);
              v = unfilter_pixel(l.filter, raw, l.cur, b, cc);
              uint8_t* px = pixels + ((size_t)y * W + x) * bpp;             // inside the pixel extent
              for (uint32_t k = 0; k < bpp; ++k) {
                px[swap ? 1 - k : k] = (uint8_t)(v >> (8 * k));
                l.ad.byte((raw >> (8 * k)) & 255u);
              }
              if (r == L - 1) {
                const Slot s{v, (int64_t)p * CGAN_PNG_MAX_DIM + x, chunk};
                if (j + 1 < waves) ring[(size_t)((j + 1) % waves) * ring_words + unf_ring_index(x, ring_words)] = s;
                else above[unf_above_index(x)] = s;
              }
            }
            l.prev = l.cur, l.cur = v;
          }
        }
      }
    }
    for (int j = 0; j < waves; ++j)
      for (int r = 0; r < L; ++r) {
        const int y = unf_row(p, j, r, waves);
        if (y < H) lanes[j * L + r].ad.end_piece(total - (uint32_t)(y + 1) * (1 + rb));
      }
  }
  uint32_t s1 = 0, s2 = 0;
  bool bad_filter = false;
  for (int i = 0; i < waves * L; ++i) {
    s1 = (s1 + lanes[i].ad.s1) % ADLER_MOD, s2 = (s2 + lanes[i].ad.s2) % ADLER_MOD;
    bad_filter = bad_filter || lanes[i].bad;
  }
  delete[] shifted, delete[] lanes, delete[] ring, delete[] above;
  if (rc) return rc;
  *status = CGAN_PNG_OK;
  why[0] = 0;
  if (bad_filter || adler_value(s1, s2, total) != trailer) {
    *status = CGAN_PNG_CORRUPT;
    snprintf(why, why_len, "%s", bad_filter ? "a filter byte above 4" : "Adler-32 mismatch");
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

// The lane-parallel inflate on the host: inflate_lanes_kernel's rounds with the lanes and the passes taken one
// after the other -- in every pass first every lane whose entry changed decodes, then every lane looks at its predecessor, as
// the wave does -- and the commit token by token.  subseq_bits = 0 is the serial form (host_run).  The status is host_decode's:
// the unfilter runs into a buffer of its own for the Adler-32 and the filter bytes' sake.  *trailer: the stream's Adler-32.
//   stats[LANES_STATS]: windows, passes in all, the most passes of one window, windows ended by a lane's cap, tokens committed
inline int host_inflate_lanes(const uint8_t* stream, const cgan_png_desc* desc, int32_t subseq_bits, int32_t lane_tokens, uint8_t* inflated,
                              uint32_t* trailer, uint32_t* stats, int32_t* status, char* why, size_t why_len) {
  if (!stream || !desc || !inflated || !trailer || !stats || !status) return snprintf(why, why_len, "null pointer"), -1;
  if (!desc_ok(*desc)) return snprintf(why, why_len, "not a descriptor the parser produces"), -1;
  if (!lanes_params_ok(subseq_bits, lane_tokens))
    return snprintf(why, why_len, "subseq_bits = %d, lane_tokens = %d: 0 or a multiple of 32 up to %u, and 1 .. %u, expected", subseq_bits,
                    lane_tokens, SUBSEQ_BITS_MAX, LANE_SLOTS), -1;
  const cgan_png_desc& d = *desc;
  const uint32_t S = (uint32_t)subseq_bits, cap = (uint32_t)lane_tokens, limit = inflated_bytes(d);
  *status = CGAN_PNG_OK, *trailer = 0;
  why[0] = 0;
  for (int k = 0; k < LANES_STATS; ++k) stats[k] = 0;
  Inflate s;
  Tables* t = new Tables;
  s.start(stream, d.stream_bytes, limit);
  if (S == 0) {
    host_run(s, *t, stream, inflated);
  } else {
    Token* slot = new Token[LANES * LANE_SLOTS];
    Token one[1];
    uint32_t entry[LANES];
    SubExit ex[LANES];
    bool changed[LANES];
    uint32_t pos = 0;
    while (s.phase != PHASE_DONE && !s.err) {
      if (s.phase != PHASE_CODES) {                      // serially: headers, stored blocks, the trailer
        s.out = pos;
        if (phase_step(s, *t, one, 0)) pos = host_execute(one[0], stream, inflated, pos);
        continue;
      }
      const uint32_t P = (uint32_t)s.r.used();
      for (uint32_t i = 0; i < LANES; ++i) entry[i] = lane_first_entry(P, i, S), changed[i] = true;
      uint32_t passes = 0;
      for (bool any = true; any && passes < LANES;) {
        ++passes;
        for (uint32_t i = 0; i < LANES; ++i)
          if (changed[i]) {
            const uint32_t end = lane_end(P, i, S);
            ex[i] = entry[i] >= end ? SubExit{entry[i], SUB_NONE, 0} : decode_subseq(stream, d.stream_bytes, entry[i], *t, end, slot, i, cap);
          }
        any = false, changed[0] = false;
        for (uint32_t i = LANES - 1; i >= 1; --i) {      // every lane reads its predecessor's exit of this pass
          changed[i] = ex[i - 1].flag == SUB_NONE && ex[i - 1].bit != entry[i];
          if (changed[i]) entry[i] = ex[i - 1].bit, any = true;
        }
      }
      uint32_t c = 0;
      while (c < LANES - 1 && ex[c].flag == SUB_NONE) ++c;
      stats[STAT_WINDOWS]++, stats[STAT_PASSES] += passes;
      if (passes > stats[STAT_MAX_PASSES]) stats[STAT_MAX_PASSES] = passes;
      if (ex[c].flag == SUB_FULL) stats[STAT_FULL_WINDOWS]++;
      for (uint32_t i = 0; i <= c && !s.err; ++i)
        for (uint32_t j = 0; j < ex[i].count && !s.err; ++j) {
          const Token k = slot[slot_index(i, j)];
          if (token_refused(k, pos, limit)) s.err = CGAN_PNG_CORRUPT;
          else pos = host_execute(k, stream, inflated, pos), stats[STAT_TOKENS]++;
        }
      if (ex[c].flag == SUB_BAD) s.err = CGAN_PNG_CORRUPT;
      if (s.err) break;
      s.r.seat_bit(ex[c].bit);
      if (ex[c].flag == SUB_EOB) s.phase = s.last ? PHASE_TRAILER : PHASE_HEADER;
    }
    delete[] slot;
  }
  delete t;
  if (s.err) {
    *status = CGAN_PNG_CORRUPT;
    return snprintf(why, why_len, "an invalid deflate stream"), 0;
  }
  *trailer = s.adler;
  uint8_t* pixels = new uint8_t[pixel_bytes(d)];
  const int rc = host_unfilter(d, inflated, s.adler, pixels, status, why, why_len);
  delete[] pixels;
  return rc;
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
