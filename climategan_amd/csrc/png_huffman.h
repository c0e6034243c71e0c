// Serial Huffman-code construction for the PNG encoder's dynamic blocks (png.hip): plain functions on plain
// arrays, the same text for the host (cgan_png_huffman_lengths, tested without a GPU) and for the one lane of
// png_rows_kernel that runs them.
//
//   counts -> code lengths, limited    sort_counts + lengths_from_sorted
//   lengths -> codes                   codes_from_lengths (RFC 1951 3.2.2, returned bit-reversed: bit 0 enters the stream first)
//   length sequence -> header tokens   header_tokens (run lengths with the symbols 16, 17, 18 of RFC 1951 3.2.7)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PNG_HD __host__ __device__
#else
#define PNG_HD
#endif

namespace png_huff {

constexpr int MAX_BITS = 15;          // the longest code deflate allows (literal / length and distance alphabets)
constexpr int NUM_LITLEN = 286;       // literal / length symbols a block may use
constexpr int NUM_CL = 19;            // the code-length alphabet; its own codes have at most 7 bits
constexpr int CL_MAX_BITS = 7;

// Used symbols in ascending order of (count, symbol): sorted[k] their counts, order[k] the symbols; returns how many.
// Insertion sort: for the 19-symbol alphabet and the host; png_rows_kernel ranks the 286 in parallel instead.
PNG_HD inline int sort_counts(const uint32_t* counts, int n, uint32_t* sorted, uint16_t* order) {
  int used = 0;
  for (int s = 0; s < n; ++s) {
    const uint32_t cnt = counts[s];
    if (cnt == 0) continue;
    int k = used++;
    for (; k > 0 && sorted[k - 1] > cnt; --k) {       // equal counts stay in symbol order
      sorted[k] = sorted[k - 1];
      order[k] = order[k - 1];
    }
    sorted[k] = cnt;
    order[k] = (uint16_t)s;
  }
  return used;
}

// Code lengths of the `used` symbols of sort_counts (2 <= used <= 2^limit, limit <= MAX_BITS) into lengths[order[k]];
// the lengths of unused symbols are not touched (the caller zeroes them).  sorted[] is overwritten.
//   1. Huffman depths in place (Moffat & Katajainen, "In-place calculation of minimum-redundancy codes", 1995); on equal
//      weights a leaf is taken before an internal node, which gives the optimal code of the least depth.
//   2. Depths above the limit are cut to it; the Kraft sum, in units of 2^-limit, is then brought back to exactly
//      2^limit one unit at a time: one code leaves the limit's level and one code of the deepest level above moves down
//      a level together with it.  The result is complete, and equals step 1's where that stayed within the limit.
//   3. The lengths go to the symbols longest first in the sorted order, so ties fall by symbol index.
// One used symbol gets length 1 (an incomplete code: a complete one needs two symbols).
PNG_HD inline void lengths_from_sorted(uint32_t* sorted, const uint16_t* order, int used, int limit, uint8_t* lengths) {
  if (used <= 0) return;
  if (used == 1) {
    lengths[order[0]] = 1;
    return;
  }
  uint32_t* A = sorted;
  const int n = used;
  A[0] += A[1];
  int root = 0, leaf = 2;
  for (int next = 1; next < n - 1; ++next) {
    if (leaf >= n || A[root] < A[leaf]) {
      A[next] = A[root];
      A[root++] = (uint32_t)next;
    } else {
      A[next] = A[leaf++];
    }
    if (leaf >= n || (root < next && A[root] < A[leaf])) {
      A[next] += A[root];
      A[root++] = (uint32_t)next;
    } else {
      A[next] += A[leaf++];
    }
  }
  A[n - 2] = 0;
  for (int next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1u;
  uint32_t per_len[MAX_BITS + 1];
  for (int l = 0; l <= MAX_BITS; ++l) per_len[l] = 0;
  {
    int avbl = 1, taken = 0;
    uint32_t depth = 0;
    root = n - 2;
    while (avbl > 0) {
      while (root >= 0 && A[root] == depth) {
        ++taken;
        --root;
      }
      const uint32_t l = depth < (uint32_t)limit ? depth : (uint32_t)limit;
      while (avbl > taken) {
        ++per_len[l];
        --avbl;
      }
      avbl = 2 * taken;
      ++depth;
      taken = 0;
    }
  }
  uint32_t total = 0;
  for (int l = limit; l >= 1; --l) total += per_len[l] << (limit - l);
  while (total > (1u << limit)) {
    --per_len[limit];
    for (int l = limit - 1; l >= 1; --l) {
      if (per_len[l]) {
        --per_len[l];
        per_len[l + 1] += 2;
        break;
      }
    }
    --total;
  }
  int k = 0;                                          // sorted position 0 is the rarest symbol: the longest code
  for (int l = limit; l >= 1; --l)
    for (uint32_t j = 0; j < per_len[l]; ++j) lengths[order[k++]] = (uint8_t)l;
}

PNG_HD inline uint32_t reverse_bits(uint32_t v, uint32_t nbits) {
  v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
  v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
  v = ((v & 0x0F0Fu) << 4) | ((v >> 4) & 0x0F0Fu);
  v = ((v & 0x00FFu) << 8) | ((v >> 8) & 0x00FFu);
  return v >> (16u - nbits);
}

// canonical codes of RFC 1951 3.2.2 for lengths[0 .. n) (0: no code), bit-reversed
PNG_HD inline void codes_from_lengths(const uint8_t* lengths, int n, uint16_t* codes) {
  uint32_t next_code[MAX_BITS + 2];
  for (int l = 0; l <= MAX_BITS + 1; ++l) next_code[l] = 0;
  for (int s = 0; s < n; ++s) ++next_code[lengths[s] + 1];          // next_code[l + 1] = number of codes of length l
  next_code[1] = 0;
  for (int l = 2; l <= MAX_BITS; ++l) next_code[l] = (next_code[l] + next_code[l - 1]) << 1;
  for (int s = 0; s < n; ++s) {
    const uint32_t l = lengths[s];
    codes[s] = l ? (uint16_t)reverse_bits(next_code[l]++, l) : (uint16_t)0;
  }
}

// extra bits that follow the code-length symbols 16 (repeat the last length 3..6 times), 17 (3..10 zeros), 18 (11..138 zeros)
PNG_HD inline uint32_t cl_extra_bits(uint32_t sym) { return sym < 16u ? 0u : (sym == 16u ? 2u : (sym == 17u ? 3u : 7u)); }

// The order in which a block header lists the lengths of the code-length code (RFC 1951 3.2.7); HCLEN trims its tail.
PNG_HD inline int cl_order(int k) {
  constexpr uint8_t o[NUM_CL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  return o[k];
}

// The sequence of code lengths of a block header (literal / length lengths, then the distance lengths) -> tokens
// (symbol | extra value << 5), at most n of them, and cl_counts[19]: how often each code-length symbol occurs.
// Zeros: runs of 11..138 as symbol 18, of 3..10 as 17; other lengths: the length once, then repeats of 3..6 as symbol 16;
// what is left of a run below 3 goes out as plain lengths.
PNG_HD inline int header_tokens(const uint8_t* seq, int n, uint16_t* tokens, uint32_t* cl_counts) {
  for (int s = 0; s < NUM_CL; ++s) cl_counts[s] = 0;
  int nt = 0;
  for (int i = 0; i < n;) {
    const uint32_t v = seq[i];
    int run = 1;
    while (i + run < n && seq[i + run] == v) ++run;
    i += run;
    if (v != 0) {                                     // symbol 16 repeats the PREVIOUS length: the first goes out plain
      tokens[nt++] = (uint16_t)v;
      ++cl_counts[v];
      --run;
    }
    while (run > 0) {
      uint32_t sym, extra = 0;
      int take;
      if (v == 0 && run >= 11) {
        take = run < 138 ? run : 138;
        sym = 18;
        extra = (uint32_t)take - 11u;
      } else if (v == 0 && run >= 3) {
        take = run;
        sym = 17;
        extra = (uint32_t)take - 3u;
      } else if (v != 0 && run >= 3) {
        take = run < 6 ? run : 6;
        sym = 16;
        extra = (uint32_t)take - 3u;
      } else {
        take = 1;
        sym = v;
      }
      tokens[nt++] = (uint16_t)(sym | (extra << 5));
      ++cl_counts[sym];
      run -= take;
    }
  }
  return nt;
}

}  // namespace png_huff
