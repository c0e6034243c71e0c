// The PNG decoder's core (png_decode.hip): plain functions on plain arrays, the same text for the host
// (cgan_png_parse_host, cgan_png_decode_host: tested and run under sanitizers without a GPU) and for the kernels.
//
//   parse            a file's bytes -> cgan_png_desc (host only): chunks, the IHDR CRC, the zlib header
//   copy_stream      the IDAT payloads one behind the other (host only)
//   Reader           the bit reader: a 64-bit window refilled a word at a time, never a byte outside the stream
//   Tables           the code tables of the block being decoded: a direct table for short codes, canonical counts behind it
//   decode_tokens    the inflate step: the stream from where it stands -> a batch of tokens (literal, match, stored run)
//   decode_subseq    the same step for one lane of a wave: the tokens that begin in a range of bits, and the
//                    window rule's few shared functions
//   Inflate::start_row   the same step on one row's chunk of a row-framed file: the reader bounded to the chunk
//   unfilter_pixel   the five predictors on up to four bytes at once, selected by the row's filter byte
//   Adler            the checksum as sums that can be split over rows and added up
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "climategan_hip.h"

#if defined(__HIPCC__)
#define PNG_HD __host__ __device__
#else
#define PNG_HD
#endif

namespace png_dec {

constexpr uint32_t MAX_STREAM_BYTES = 1u << 28;      // bit positions stay below 2^31
constexpr uint32_t WINDOW = 32768;                   // the farthest a match reaches back
constexpr uint32_t ADLER_MOD = 65521;

// ---- the descriptor --------------------------------------------------------------------------------------------------------
PNG_HD inline uint32_t bytes_per_pixel(const cgan_png_desc& d) { return (uint32_t)d.channels * (uint32_t)(d.bit_depth / 8); }
PNG_HD inline uint32_t row_bytes(const cgan_png_desc& d) { return (uint32_t)d.width * bytes_per_pixel(d); }
PNG_HD inline uint32_t inflated_bytes(const cgan_png_desc& d) { return (uint32_t)d.height * (1u + row_bytes(d)); }   // < 2^29
PNG_HD inline uint32_t pixel_bytes(const cgan_png_desc& d) { return (uint32_t)d.height * row_bytes(d); }
PNG_HD inline uint32_t table_words(const cgan_png_desc& d) { return d.rows ? d.rows + 1u : 0u; }       // of a row-framed candidate
// what the device call and the host twin take: the ranges every index below relies on
PNG_HD inline bool desc_ok(const cgan_png_desc& d) {
  if (d.width < 1 || d.width > CGAN_PNG_MAX_DIM || d.height < 1 || d.height > CGAN_PNG_MAX_DIM) return false;
  if (!((d.bit_depth == 8 && (d.channels == 1 || d.channels == 3 || d.channels == 4)) || (d.bit_depth == 16 && d.channels == 1)))
    return false;
  if (d.rows != 0 && d.rows != (uint32_t)d.height) return false;
  return d.stream_bytes >= 2 && d.stream_bytes <= MAX_STREAM_BYTES;
}
// a candidate's table: row k's bytes are [table[k], table[k + 1]), the tail's [table[rows], stream_bytes)
PNG_HD inline bool table_ok(const cgan_png_desc& d, const uint32_t* table) {
  if (table[0] != 2) return false;
  for (uint32_t k = 0; k < d.rows; ++k)
    if (table[k + 1] <= table[k]) return false;
  return table[d.rows] <= d.stream_bytes;
}

// ---- the bit reader --------------------------------------------------------------------------------------------------------
// Deflate packs its bits from the least significant bit of every byte.  `win` holds the next `n` bits, the next one lowest.
// A refill appends the next four bytes as one word (the stream's first byte is 4-byte aligned in the device's blob); the last,
// partial word is put together from its bytes, and behind the stream's end zeros enter: used() then runs past 8 * len, which
// every caller checks before it trusts what it read.
struct Reader {
  const uint8_t* p;
  uint32_t len, next, n;       // next: the byte the next word starts at, a multiple of 4
  uint64_t win;
  PNG_HD void start(const uint8_t* stream, uint32_t bytes) { p = stream, len = bytes, next = 0, n = 0, win = 0; }
  // re-seat at byte `at`: at the word that holds the byte, the bits before the byte dropped
  PNG_HD void seat(uint32_t at) {
    next = at & ~3u, n = 0, win = 0;
    refill();
    take(8 * (at & 3u));
  }
  // re-seat at bit `at` of the stream (at <= 2^31 + 2^16; behind the stream's end zeros enter, as in a refill)
  PNG_HD void seat_bit(uint32_t at) {
    seat(at >> 3);
    take(at & 7u);                                         // seat leaves at least 8 bits
  }
  PNG_HD uint32_t word() const {
    uint32_t w = 0;
    if (next + 4 <= len) {
#if defined(__HIP_DEVICE_COMPILE__)
      w = *reinterpret_cast<const uint32_t*>(p + next);
#else
      memcpy(&w, p + next, 4);
#endif
    } else {
      for (uint32_t k = 0; k < 4; ++k)
        if (next + k < len) w |= (uint32_t)p[next + k] << (8 * k);
    }
    return w;
  }
  PNG_HD void refill() {                                   // afterwards 33 <= n <= 64
    if (n <= 32) {
      win |= (uint64_t)word() << n;
      n += 32, next += 4;
    }
  }
  PNG_HD uint32_t peek(uint32_t k) const { return (uint32_t)win & ((1u << k) - 1u); }     // 0 <= k <= 16
  PNG_HD void take(uint32_t k) { win >>= k, n -= k; }                                    // k <= n
  PNG_HD uint32_t bits(uint32_t k) {
    const uint32_t v = peek(k);
    take(k);
    return v;
  }
  PNG_HD uint64_t used() const { return 8ull * next - n; }                               // bits consumed so far
  PNG_HD bool past_end() const { return used() > 8ull * len; }
};

// ---- the code tables -------------------------------------------------------------------------------------------------------
// A code table in two forms: fast[] maps the next FAST bits to (symbol << 4 | length) for codes of at most FAST bits, 0
// otherwise; count[] / symbol[] are the canonical form (how many codes of each length, the symbols in code order) that decodes
// the longer ones a bit at a time.  Every index is masked or bounded by the array's size.
constexpr uint32_t FAST_LIT = 10, FAST_DIST = 8, MAX_LIT = 288, MAX_DIST = 32;
template <uint32_t FAST, uint32_t NSYM>
struct Code {
  uint16_t fast[1u << FAST];
  uint16_t count[16];
  uint16_t symbol[NSYM];
};
struct Tables {
  Code<FAST_LIT, MAX_LIT> lit;
  Code<FAST_DIST, MAX_DIST> dist;
  uint8_t lens[MAX_LIT + MAX_DIST];      // the code lengths of the block's header while it is read
};

// lens[0 .. n) -> the table.  Returns 0 for a complete code, > 0 for an incomplete one (the code space left), < 0 for an
// over-subscribed one, as zlib's rule needs them told apart.
template <uint32_t FAST, uint32_t NSYM>
PNG_HD inline int build_code(Code<FAST, NSYM>& c, const uint8_t* lens, uint32_t n) {
  uint16_t offs[16];
  for (int l = 0; l < 16; ++l) c.count[l] = 0;
  for (uint32_t s = 0; s < n; ++s) c.count[lens[s] & 15]++;
  for (uint32_t i = 0; i < (1u << FAST); ++i) c.fast[i] = 0;
  int left = 1;
  for (int l = 1; l < 16; ++l) {
    left = (left << 1) - (int)c.count[l];
    if (left < 0) return left;
  }
  offs[1] = 0;
  for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + c.count[l]);
  for (uint32_t s = 0; s < n; ++s)
    if (lens[s] & 15) c.symbol[offs[lens[s] & 15]++ % NSYM] = (uint16_t)s;
  // the direct table: the canonical codes in order, each reversed (the stream has a code's first bit lowest)
  uint32_t code = 0, k = 0;
  for (uint32_t l = 1; l <= FAST; ++l) {
    for (uint32_t i = 0; i < c.count[l]; ++i, ++k, ++code) {
      uint32_t r = 0;
      for (uint32_t b = 0; b < l; ++b) r |= ((code >> b) & 1u) << (l - 1 - b);
      const uint16_t e = (uint16_t)((c.symbol[k % NSYM] << 4) | l);
      for (uint32_t at = r; at < (1u << FAST); at += 1u << l) c.fast[at] = e;
    }
    code <<= 1;
  }
  return left;
}

// zlib's rule for a code that leaves code space unused: no code at all, or a single code of one bit
template <uint32_t FAST, uint32_t NSYM>
PNG_HD inline bool incomplete_ok(const Code<FAST, NSYM>& c, uint32_t n) {
  const uint32_t used = n - c.count[0];
  return used == 0 || (used == 1 && c.count[1] == 1);
}

// the next symbol, or -1 where the bits are no code of the table (an incomplete code's unused pattern)
template <uint32_t FAST, uint32_t NSYM>
PNG_HD inline int decode_symbol(const Code<FAST, NSYM>& c, Reader& r) {
  const uint32_t e = c.fast[r.peek(FAST) & ((1u << FAST) - 1u)];
  if (e) {
    r.take(e & 15u);
    return (int)(e >> 4);
  }
  uint32_t w = r.peek(15);
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= 15; ++l) {
    code |= (int)(w & 1u);
    w >>= 1;
    const int count = c.count[l];
    if (code - count < first) {
      r.take((uint32_t)l);
      return c.symbol[(uint32_t)(index + (code - first)) % NSYM];
    }
    index += count, first += count;
    first <<= 1, code <<= 1;
  }
  return -1;
}

PNG_HD inline void fixed_lengths(uint8_t* lens) {
  for (int s = 0; s < 144; ++s) lens[s] = 8;
  for (int s = 144; s < 256; ++s) lens[s] = 9;
  for (int s = 256; s < 280; ++s) lens[s] = 7;
  for (int s = 280; s < 288; ++s) lens[s] = 8;
  for (int s = 0; s < 32; ++s) lens[288 + s] = 5;
}

// ---- the inflate step ------------------------------------------------------------------------------------------------------
// A token is what the stream says to append: one literal byte, `len` bytes from `arg` bytes back (a match; arg < len repeats),
// or `len` bytes of the stream itself from its byte `arg` (a run of a stored block).
constexpr uint32_t TOK_LITERAL = 0, TOK_MATCH = 1, TOK_STORED = 2;
struct Token {
  uint16_t len;
  uint8_t kind, lit;
  uint32_t arg;
};
constexpr uint32_t PHASE_HEADER = 0, PHASE_CODES = 1, PHASE_STORED = 2, PHASE_TRAILER = 3, PHASE_DONE = 4;
// MODE_STREAM: a whole zlib stream.  MODE_ROW: one row's chunk of a row-framed file -- whole blocks, none of them final, the
// last a stored block that ends on the chunk's last byte with the row complete (PHASE_DONE then).  MODE_TAIL: the chunk
// behind the last row -- blocks that produce nothing up to the final one, then the trailer.
constexpr uint32_t MODE_STREAM = 0, MODE_ROW = 1, MODE_TAIL = 2;
struct Inflate {
  Reader r;
  uint32_t phase, last, stored_left, stored_at, mode;
  uint32_t out, limit;         // bytes produced so far; the bytes the image has
  uint32_t adler;              // the trailer, once PHASE_DONE
  uint32_t err;
  PNG_HD void start(const uint8_t* stream, uint32_t bytes, uint32_t out_limit) {
    r.start(stream, bytes);
    r.refill();
    r.take(16);                // the zlib header, checked by the parser
    phase = PHASE_HEADER, last = 0, stored_left = 0, stored_at = 0, out = 0, limit = out_limit, adler = 0, err = 0;
    mode = MODE_STREAM;
  }
  // Row k of a candidate (k = d.rows: the tail): the stream's bytes [begin, end), begin anywhere in a word.  The reader's end is
  // the chunk's, so nothing behind it is read or taken for a stored run; `out` counts from the row's first byte, so the check
  // of a match's distance against `out` refuses a match that reaches in front of the row.  begin <= end <= the stream's bytes.
  PNG_HD void start_row(const uint8_t* stream, uint32_t begin, uint32_t end, uint32_t out_limit, uint32_t row_mode) {
    r.start(stream, end);
    r.seat(begin);
    phase = PHASE_HEADER, last = 0, stored_left = 0, stored_at = 0, out = 0, limit = out_limit, adler = 0, err = 0;
    mode = row_mode;
  }
};

PNG_HD inline uint32_t length_base(uint32_t s) {           // s = symbol - 257, 0 .. 28
  constexpr uint16_t t[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
  return t[s < 29 ? s : 28];
}
PNG_HD inline uint32_t length_extra(uint32_t s) { return (s < 8 || s >= 28) ? 0u : (s - 4) / 4; }
PNG_HD inline uint32_t dist_base(uint32_t s) {             // s = 0 .. 29
  constexpr uint16_t t[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
  return t[s < 30 ? s : 29];
}
PNG_HD inline uint32_t dist_extra(uint32_t s) { return s < 4 ? 0u : (s - 2) / 2; }

// a block's header: BFINAL, BTYPE and what follows them up to the first symbol.  Sets t and the phase; false: corrupt.
PNG_HD inline bool block_header(Inflate& s, Tables& t) {
  Reader& r = s.r;
  r.refill();
  s.last = r.bits(1);
  const uint32_t type = r.bits(2);
  if (type == 3) return false;
  if (type == 0) {
    r.take(r.n & 7u);                                      // n and the bit position agree mod 8: words are whole bytes
    r.refill();
    const uint32_t len = r.bits(16), nlen = r.bits(16);
    if (r.past_end() || (len ^ nlen) != 0xFFFFu) return false;
    // the payload starts on a byte: hand the window's whole bytes back and restart behind the run
    s.stored_at = (uint32_t)(r.used() / 8);
    s.stored_left = len;
    if ((uint64_t)s.stored_at + len > r.len) return false;
    s.phase = PHASE_STORED;
    return true;
  }
  if (type == 1) {
    fixed_lengths(t.lens);
    build_code(t.lit, t.lens, 288);
    build_code(t.dist, t.lens + 288, 30);
    s.phase = PHASE_CODES;
    return true;
  }
  const uint32_t hlit = r.bits(5) + 257, hdist = r.bits(5) + 1, hclen = r.bits(4) + 4;
  if (hlit > 286 || hdist > 30) return false;
  constexpr uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  uint8_t cl[19];
  for (int i = 0; i < 19; ++i) cl[i] = 0;
  for (uint32_t i = 0; i < hclen; ++i) {
    r.refill();
    cl[order[i]] = (uint8_t)r.bits(3);
  }
  // the code-length code lives in the distance table's place until the real one is built
  if (build_code(t.dist, cl, 19) != 0) return false;      // zlib: the code-length code must be complete
  uint32_t at = 0;
  while (at < hlit + hdist) {                              // every turn adds at least one length: at most 316 turns
    r.refill();
    const int sym = decode_symbol(t.dist, r);
    if (sym < 0 || r.past_end()) return false;
    if (sym < 16) {
      t.lens[at++] = (uint8_t)sym;
      continue;
    }
    uint32_t prev = 0, rep;
    if (sym == 16) {
      if (at == 0) return false;                           // nothing to repeat
      prev = t.lens[at - 1];
      rep = 3 + r.bits(2);
    } else if (sym == 17) {
      rep = 3 + r.bits(3);
    } else {
      rep = 11 + r.bits(7);
    }
    if (at + rep > hlit + hdist) return false;
    for (uint32_t k = 0; k < rep; ++k) t.lens[at++] = (uint8_t)prev;
  }
  if (r.past_end()) return false;
  if (t.lens[256] == 0) return false;                      // no end-of-block code
  uint8_t dl[MAX_DIST];
  for (uint32_t i = 0; i < MAX_DIST; ++i) dl[i] = i < hdist ? t.lens[hlit + i] : 0;
  const int ll = build_code(t.lit, t.lens, hlit);
  if (ll < 0 || (ll > 0 && !incomplete_ok(t.lit, hlit))) return false;
  const int dd = build_code(t.dist, dl, hdist);
  if (dd < 0 || (dd > 0 && !incomplete_ok(t.dist, hdist))) return false;
  s.phase = PHASE_CODES;
  return true;
}

// One step of a phase other than PHASE_CODES: a block's header, a stored block's run (a token, unless it is empty), the
// trailer.  Appends to tok[nt] where it has a token and returns the new count.
PNG_HD inline uint32_t phase_step(Inflate& s, Tables& t, Token* tok, uint32_t nt) {
  Reader& r = s.r;
  if (s.phase == PHASE_HEADER) {
    if (!block_header(s, t) || r.past_end()) s.err = CGAN_PNG_CORRUPT;
    if (s.mode == MODE_ROW && s.last) s.err = CGAN_PNG_CORRUPT;      // a final block inside a row's chunk
    return nt;
  }
  if (s.phase == PHASE_STORED) {
    if (s.stored_left) {
      if (s.stored_left > s.limit - s.out) {
        s.err = CGAN_PNG_CORRUPT;
        return nt;
      }
      tok[nt++] = Token{(uint16_t)s.stored_left, (uint8_t)TOK_STORED, 0, s.stored_at};
      s.out += s.stored_left;
    }
    // restart the reader behind the run: at the word that holds the byte, the bits before the byte dropped
    const uint32_t at = s.stored_at + s.stored_left;
    r.seat(at);
    s.stored_left = 0;
    s.phase = s.last ? PHASE_TRAILER : PHASE_HEADER;
    if (s.mode == MODE_ROW && at == r.len) {                         // the row-end rule: the chunk ends with this stored block
      if (s.out != s.limit) s.err = CGAN_PNG_CORRUPT;
      s.phase = PHASE_DONE;
    }
    return nt;
  }
  // PHASE_TRAILER
  r.take(r.n & 7u);
  r.refill();
  uint32_t a = 0;
  for (int k = 0; k < 4; ++k) a = (a << 8) | r.bits(8);
  if (r.past_end() || s.out != s.limit) s.err = CGAN_PNG_CORRUPT;
  s.adler = a;
  s.phase = PHASE_DONE;
  return nt;
}

// Decodes until `max_tok` tokens stand in tok[], the stream is done (PHASE_DONE) or an error is found (s.err).  Every turn of
// the loop consumes at least one bit of the stream or leaves the loop, and a reader that has run past the stream's end is an
// error, so the turns are bounded by 8 * stream bytes whatever the bytes are.
PNG_HD inline uint32_t decode_tokens(Inflate& s, Tables& t, Token* tok, uint32_t max_tok) {
  uint32_t nt = 0;
  Reader& r = s.r;
  while (nt < max_tok && s.phase != PHASE_DONE && !s.err) {
    if (s.phase != PHASE_CODES) {
      nt = phase_step(s, t, tok, nt);
      continue;
    }
    r.refill();
    const int sym = decode_symbol(t.lit, r);
    if (sym < 0 || sym > 285 || r.past_end()) {
      s.err = CGAN_PNG_CORRUPT;
      continue;
    }
    if (sym < 256) {
      if (s.out >= s.limit) {
        s.err = CGAN_PNG_CORRUPT;
        continue;
      }
      tok[nt++] = Token{1, (uint8_t)TOK_LITERAL, (uint8_t)sym, 0};
      s.out += 1;
      continue;
    }
    if (sym == 256) {
      s.phase = s.last ? PHASE_TRAILER : PHASE_HEADER;
      continue;
    }
    const uint32_t ls = (uint32_t)sym - 257u;
    const uint32_t len = length_base(ls) + r.bits(length_extra(ls));
    r.refill();
    const int ds = decode_symbol(t.dist, r);
    if (ds < 0 || ds > 29) {
      s.err = CGAN_PNG_CORRUPT;
      continue;
    }
    const uint32_t dist = dist_base((uint32_t)ds) + r.bits(dist_extra((uint32_t)ds));
    if (r.past_end() || dist > s.out || len > s.limit - s.out) {
      s.err = CGAN_PNG_CORRUPT;
      continue;
    }
    tok[nt++] = Token{(uint16_t)len, (uint8_t)TOK_MATCH, 0, dist};
    s.out += len;
  }
  return nt;
}

// ---- the inflate step across a wave's lanes ---------------------------------------------------------------------
// Inside a block of Huffman codes the state of a decode is one number, the bit at which the next token begins, and a decode
// that starts at a wrong bit falls into step with the right one after a few tokens.  A window of LANES * S bits starts at a
// committed bit P; lane i owns the bits [P + i * S, P + (i + 1) * S) and decodes the tokens that BEGIN there (decode_subseq)
// into its own slots: lane 0 from P, lane i > 0 first from its own first bit.  In every pass each lane whose entry changed
// decodes again; then lane i takes the exit bit of lane i - 1 as its entry if that lane ran to its range's end (SUB_NONE).  An
// entry at or behind the lane's own end leaves the lane empty and is passed on.  After pass k lanes 0 .. k - 1 hold what the
// serial decode gives, so no entry changes after at most LANES passes.  The lanes up to and including the first whose flag is
// not SUB_NONE are committed, and P moves to that lane's exit bit.  What needs the output position (a match's distance, the
// extent's end) is checked when the tokens are committed (token_refused), not here.
constexpr uint32_t LANES = 64;
constexpr uint32_t LANE_SLOTS = 48;                   // token slots per lane: the most lane_tokens can be (24 KiB of LDS)
constexpr uint32_t SUBSEQ_BITS_MAX = 256;
#ifndef CGAN_PNG_SUBSEQ_BITS
#define CGAN_PNG_SUBSEQ_BITS 96
#endif
#ifndef CGAN_PNG_LANE_TOKENS
#define CGAN_PNG_LANE_TOKENS 48
#endif
constexpr uint32_t SUBSEQ_BITS_DEFAULT = CGAN_PNG_SUBSEQ_BITS, LANE_TOKENS_DEFAULT = CGAN_PNG_LANE_TOKENS;
// why a lane stopped: its range's end; behind an end-of-block symbol; an invalid symbol or the stream's end; `cap` tokens
constexpr uint32_t SUB_NONE = 0, SUB_EOB = 1, SUB_BAD = 2, SUB_FULL = 3;
PNG_HD inline bool lanes_params_ok(int32_t subseq_bits, int32_t lane_tokens) {      // subseq_bits 0: the serial form
  return subseq_bits >= 0 && subseq_bits <= (int32_t)SUBSEQ_BITS_MAX && subseq_bits % 32 == 0 && lane_tokens >= 1 &&
         lane_tokens <= (int32_t)LANE_SLOTS;
}
PNG_HD inline uint32_t lane_end(uint32_t P, uint32_t lane, uint32_t S) { return P + (lane + 1u) * S; }     // P <= 2^31: no overflow
PNG_HD inline uint32_t lane_first_entry(uint32_t P, uint32_t lane, uint32_t S) { return P + lane * S; }
// lane `lane`'s token j of a window's slots: the lanes side by side, so that a wave's lanes write neighbouring words
PNG_HD inline uint32_t slot_index(uint32_t lane, uint32_t j) { return (j % LANE_SLOTS) * LANES + (lane % LANES); }

struct SubExit {
  uint32_t bit, flag, count;
};
// The tokens that begin in [e, end) of the stream, at most cap <= LANE_SLOTS of them, into slot[slot_index(lane, 0 ..)].  A
// length symbol, its extra bits, the distance symbol and its extra bits are one token.  -> the exit bit (SUB_NONE, SUB_FULL:
// where the next token begins; SUB_EOB: behind the end-of-block symbol), the flag and the count.  Writes nothing but the
// slots, reads nothing outside the stream (Reader::word); every turn consumes a bit or returns.
PNG_HD inline SubExit decode_subseq(const uint8_t* stream, uint32_t stream_bytes, uint32_t e, const Tables& t, uint32_t end, Token* slot,
                                    uint32_t lane, uint32_t cap) {
  Reader r;
  r.start(stream, stream_bytes);
  r.seat_bit(e);
  uint32_t nt = 0;
  for (;;) {
    const uint32_t at = (uint32_t)r.used();
    if (at >= end) return SubExit{at, SUB_NONE, nt};
    if (nt >= cap) return SubExit{at, SUB_FULL, nt};
    r.refill();
    const int sym = decode_symbol(t.lit, r);
    if (sym < 0 || sym > 285 || r.past_end()) return SubExit{at, SUB_BAD, nt};
    if (sym < 256) {
      slot[slot_index(lane, nt++)] = Token{1, (uint8_t)TOK_LITERAL, (uint8_t)sym, 0};
      continue;
    }
    if (sym == 256) return SubExit{(uint32_t)r.used(), SUB_EOB, nt};
    const uint32_t ls = (uint32_t)sym - 257u;
    const uint32_t len = length_base(ls) + r.bits(length_extra(ls));
    r.refill();
    const int ds = decode_symbol(t.dist, r);
    if (ds < 0 || ds > 29) return SubExit{at, SUB_BAD, nt};
    const uint32_t dist = dist_base((uint32_t)ds) + r.bits(dist_extra((uint32_t)ds));
    if (r.past_end()) return SubExit{at, SUB_BAD, nt};
    slot[slot_index(lane, nt++)] = Token{(uint16_t)len, (uint8_t)TOK_MATCH, 0, dist};
  }
}
// the commit's checks of a token that goes to byte `at` of an extent of `limit` bytes: at <= limit
PNG_HD inline bool token_refused(const Token& k, uint32_t at, uint32_t limit) {
  return (k.kind == TOK_MATCH && k.arg > at) || k.len > limit - at;
}
// what the twin reports beside the bytes (cgan_png_inflate_lanes_host)
constexpr int LANES_STATS = 5;
constexpr int STAT_WINDOWS = 0, STAT_PASSES = 1, STAT_MAX_PASSES = 2, STAT_FULL_WINDOWS = 3, STAT_TOKENS = 4;

// ---- the unfilter arithmetic -----------------------------------------------------------------------------------------------
PNG_HD inline uint32_t paeth(uint32_t a, uint32_t b, uint32_t c) {
  const int p = (int)a + (int)b - (int)c;
  const int pa = p > (int)a ? p - (int)a : (int)a - p, pb = p > (int)b ? p - (int)b : (int)b - p,
            pc = p > (int)c ? p - (int)c : (int)c - p;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// One pixel of up to four bytes (byte k in bits 8k ..): raw as the file has it, a = the pixel to the left, b = the one above,
// c = the one above a, all reconstructed -> the reconstructed pixel.  All five predictors are computed and one is selected.
PNG_HD inline uint32_t unfilter_pixel(uint32_t filter, uint32_t raw, uint32_t a, uint32_t b, uint32_t c) {
  uint32_t out = 0;
  for (int k = 0; k < 4; ++k) {
    const uint32_t x = (raw >> (8 * k)) & 255u, ak = (a >> (8 * k)) & 255u, bk = (b >> (8 * k)) & 255u, ck = (c >> (8 * k)) & 255u;
    const uint32_t avg = (ak + bk) >> 1, pae = paeth(ak, bk, ck);
    const uint32_t pred = filter == 1 ? ak : (filter == 2 ? bk : (filter == 3 ? avg : (filter == 4 ? pae : 0u)));
    out |= ((x + pred) & 255u) << (8 * k);
  }
  return out;
}

// ---- the wide unfilter's schedule ------------------------------------------------------------------------------
// One workgroup of `waves` waves per file.  In pass p, wave j, lane r owns row p * 64 * waves + 64 * j + r; in step s of a pass
// that lane is at pixel s - unf_wave_offset(j) - r.  Lane 0 of wave j > 0 reads the row above it from a ring that lane 63 of
// wave j - 1 wrote unf lag + 1 steps earlier: lag is a multiple of UNF_PREFETCH and at least that, so the write lies in an
// earlier chunk of UNF_PREFETCH steps -- in front of the barrier that ends it -- and a ring of at least lag + 1 + UNF_PREFETCH
// words is not written again before the chunk of the read is over.  Every count below depends on the descriptor alone.
constexpr int UNF_LANES = 64;                        // one wave
constexpr int UNF_PREFETCH = 8;                      // steps of the wavefront between two barriers; their bytes are loaded together
constexpr int UNF_MAX_WAVES = 16;
PNG_HD inline bool unf_params_ok(int waves, int lag) {
  return waves >= 1 && waves <= UNF_MAX_WAVES && lag >= UNF_PREFETCH && lag % UNF_PREFETCH == 0 && lag <= 8 * UNF_PREFETCH;
}
PNG_HD inline int unf_wave_offset(int wave, int lag) { return wave * (UNF_LANES + lag); }   // steps wave `wave` runs behind wave 0
PNG_HD inline uint32_t unf_steps(int width, int waves, int lag) {
  return (uint32_t)(width + UNF_LANES - 1 + unf_wave_offset(waves - 1, lag));
}
PNG_HD inline uint32_t unf_chunks(int width, int waves, int lag) { return (unf_steps(width, waves, lag) + UNF_PREFETCH - 1) / UNF_PREFETCH; }
PNG_HD inline uint32_t unf_passes(int height, int waves) { return ((uint32_t)height + UNF_LANES * waves - 1) / (uint32_t)(UNF_LANES * waves); }
PNG_HD inline int unf_row(uint32_t pass, int wave, int lane, int waves) { return (int)pass * UNF_LANES * waves + UNF_LANES * wave + lane; }
PNG_HD constexpr uint32_t unf_ring_words(int lag) {                                          // a power of two
  uint32_t n = 1;
  while (n < (uint32_t)(lag + 1 + UNF_PREFETCH)) n <<= 1;
  return n;
}
PNG_HD inline uint32_t unf_ring_index(int x, uint32_t words) { return (uint32_t)x & (words - 1u); }
PNG_HD inline uint32_t unf_above_index(int x) { return (uint32_t)x & (uint32_t)(CGAN_PNG_MAX_DIM - 1); }
// whether a wave has nothing to do in the chunk whose first step is t0 of its own clock: its rows lie beyond the image, or
// its lanes are all in front of the row's first pixel or behind its last.  The same in every lane of the wave.
PNG_HD inline bool unf_wave_idle(int first_row, int height, int t0, int width) {
  return first_row >= height || t0 + UNF_PREFETCH - 1 < 0 || t0 - (UNF_LANES - 1) >= width;
}

// ---- Adler-32 --------------------------------------------------------------------------------------------------------------
// adler = (s2 << 16) | s1 with s1 = 1 + sum of the bytes, s2 = N + sum over i of (N - i) * byte i, both mod 65521: linear in
// the bytes, so a piece of the stream (a row) contributes on its own and the contributions add up in any order.
struct Adler {
  uint64_t a, b;               // of the piece being walked: the sum of its bytes, the sum of its running sums
  uint32_t s1, s2;             // of the pieces finished, mod 65521
  PNG_HD void start() { a = 0, b = 0, s1 = 0, s2 = 0; }
  PNG_HD void byte(uint32_t v) { a += v, b += a; }         // a piece of at most 2^15 + 1 bytes: b < 2^39
  // the piece ends `tail` bytes before the stream's end
  PNG_HD void end_piece(uint32_t tail) {
    const uint32_t am = (uint32_t)(a % ADLER_MOD);
    s1 = (s1 + am) % ADLER_MOD;
    s2 = (uint32_t)((s2 + b % ADLER_MOD + (uint64_t)am * (tail % ADLER_MOD)) % ADLER_MOD);
    a = 0, b = 0;
  }
};
PNG_HD inline uint32_t adler_value(uint32_t s1, uint32_t s2, uint32_t total) {
  return (((s2 + total % ADLER_MOD) % ADLER_MOD) << 16) | ((s1 + 1u) % ADLER_MOD);
}

// ---- the parser (host) -----------------------------------------------------------------------------------------------------
inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
inline uint32_t crc32(const uint8_t* p, size_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  }
  return ~c;
}

// Walks the chunks.  Returns the status and fills *d for CGAN_PNG_OK; `why` says what was found otherwise.  With dst, the IDAT
// payloads are copied there one behind the other (at most dst_bytes of them).
// Row-framed candidates: exactly height + 1 IDAT chunks, the first longer than the zlib header, chunks
// 1 .. height - 1 not empty -> d->rows = height, else 0.  With table (height + 1 words), the chunks' cumulative lengths go
// there: where row k's bytes begin in the stream (row 0: behind the header) and where the tail begins.
inline int walk(const uint8_t* f, size_t n, cgan_png_desc* d, uint8_t* dst, size_t dst_bytes, char* why, size_t why_len,
                uint32_t* table = nullptr, uint32_t table_len = 0) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  memset(d, 0, sizeof(*d));
  if (n < 8 || memcmp(f, sig, 8) != 0) return snprintf(why, why_len, "not a PNG file"), CGAN_PNG_UNSUPPORTED;
  size_t at = 8;
  bool have_ihdr = false, in_idat = false, idat_over = false, apng = false;
  uint64_t stream = 0, idats = 0;
  bool framed = true;
  uint8_t head[2] = {0, 0};
  uint32_t depth = 0, colour = 0, interlace = 0, compression = 0, filter = 0, w = 0, h = 0;
  while (at < n) {
    if (n - at < 12) return snprintf(why, why_len, "a chunk runs past the file's end"), CGAN_PNG_CORRUPT;
    const uint32_t len = be32(f + at);
    const uint8_t* type = f + at + 4;
    if ((uint64_t)len + 12 > n - at) return snprintf(why, why_len, "a chunk runs past the file's end"), CGAN_PNG_CORRUPT;
    const uint8_t* data = f + at + 8;
    const bool is_ihdr = memcmp(type, "IHDR", 4) == 0, is_idat = memcmp(type, "IDAT", 4) == 0;
    if (!have_ihdr) {
      if (!is_ihdr || len != 13) return snprintf(why, why_len, "the first chunk is not IHDR"), CGAN_PNG_CORRUPT;
      if (crc32(type, 4 + 13) != be32(data + 13)) return snprintf(why, why_len, "bad IHDR CRC"), CGAN_PNG_CORRUPT;
      w = be32(data), h = be32(data + 4), depth = data[8], colour = data[9], compression = data[10], filter = data[11],
      interlace = data[12];
      have_ihdr = true;
    } else if (is_idat) {
      if (idat_over) return snprintf(why, why_len, "IDAT chunks are not consecutive"), CGAN_PNG_CORRUPT;
      in_idat = true;
      if (idats == 0 ? len <= 2 : (idats < h && len == 0)) framed = false;
      if (table && idats < table_len) table[idats] = idats == 0 ? 2u : (uint32_t)(stream < MAX_STREAM_BYTES ? stream : MAX_STREAM_BYTES);
      ++idats;
      for (uint32_t k = 0; k < len && stream + k < 2; ++k) head[stream + k] = data[k];
      if (dst && len) {
        if (stream + len > dst_bytes) return snprintf(why, why_len, "the stream does not fit"), CGAN_PNG_CORRUPT;
        memcpy(dst + stream, data, len);
      }
      stream += len;
    } else {
      if (in_idat) idat_over = true;
      if (memcmp(type, "acTL", 4) == 0) apng = true;
      if (memcmp(type, "IEND", 4) == 0) break;
    }
    at += 12 + (size_t)len;
  }
  if (!have_ihdr) return snprintf(why, why_len, "no IHDR chunk"), CGAN_PNG_CORRUPT;
  if (apng) return snprintf(why, why_len, "an animated PNG (acTL)"), CGAN_PNG_UNSUPPORTED;
  if (compression != 0 || filter != 0) return snprintf(why, why_len, "compression or filter method not 0"), CGAN_PNG_UNSUPPORTED;
  if (interlace != 0) return snprintf(why, why_len, "Adam7 interlacing"), CGAN_PNG_UNSUPPORTED;
  if (colour == 3) return snprintf(why, why_len, "a palette file"), CGAN_PNG_UNSUPPORTED;
  if (colour == 4) return snprintf(why, why_len, "grey + alpha"), CGAN_PNG_UNSUPPORTED;
  if (colour != 0 && colour != 2 && colour != 6) return snprintf(why, why_len, "colour type %u", colour), CGAN_PNG_UNSUPPORTED;
  if (depth != 8 && depth != 16) return snprintf(why, why_len, "bit depth %u", depth), CGAN_PNG_UNSUPPORTED;
  if (depth == 16 && colour != 0) return snprintf(why, why_len, "16-bit colour"), CGAN_PNG_UNSUPPORTED;
  if (w < 1 || h < 1) return snprintf(why, why_len, "an empty image"), CGAN_PNG_CORRUPT;
  if (w > CGAN_PNG_MAX_DIM || h > CGAN_PNG_MAX_DIM)
    return snprintf(why, why_len, "%u x %u: more than %d pixels a side", w, h, CGAN_PNG_MAX_DIM), CGAN_PNG_UNSUPPORTED;
  if (!in_idat) return snprintf(why, why_len, "no IDAT chunk"), CGAN_PNG_CORRUPT;
  if (stream > MAX_STREAM_BYTES) return snprintf(why, why_len, "a stream of more than 256 MiB"), CGAN_PNG_UNSUPPORTED;
  if (stream < 2 || (head[0] & 15) != 8 || (head[0] >> 4) > 7 || (head[1] & 0x20) || (head[0] * 256u + head[1]) % 31u != 0)
    return snprintf(why, why_len, "bad zlib header"), CGAN_PNG_CORRUPT;
  d->width = (int32_t)w, d->height = (int32_t)h, d->channels = colour == 0 ? 1 : (colour == 2 ? 3 : 4), d->bit_depth = (int32_t)depth;
  d->stream_bytes = (uint32_t)stream;
  d->rows = (framed && idats == (uint64_t)h + 1) ? h : 0;
  return CGAN_PNG_OK;
}

}  // namespace png_dec
